/*
 * pawsome_exclusive.h — several targets of one video kept apart: per step the targets share out the peaks they see, so that
 * no two take the same blob.
 *
 * The reference tracks ONE target per video (src/PawsomeTracker.jl:163-169).  Several chains over one video
 * (pdog_detect_chains_indexed) are independent applications of its functor: two targets that come close see the same blobs,
 * both `findmax` calls (:59) return the same one, and from that frame on the two chains are one.  The step below is THIS
 * LIBRARY'S ADDITION, like the sub-pixel rule and the K-peaks selection it builds on (pawsome_peaks.h);
 * tests/exclusive_restatement.py states it in NumPy, and the kernel (csrc/dog_assign.hpp) and the host function are held to
 * that statement bit for bit.  Nothing changes for a caller who does not ask for it.
 *
 * THE RULE — one joint step for one GROUP of T targets (the targets of one video), T <= PDOG_EXCLUSIVE_MAX_TARGETS.
 *  Inputs.   The previous positions prev[t]; for every target the output of pdog_detect_peaks on its window at prev[t] —
 *            ij[t][0 .. k-1], peak[t][0 .. k-1], count[t], the same k and min_distance d for all —; a ratio rho in [0, 1].
 *  Admissible picks.  A target's pick 1 (list entry 0) is always admissible.  Entry q >= 1 is admissible when q < count[t],
 *            peak[t][q] > 0 and peak[t][q] >= rho_f * peak[t][0], with rho_f = (float)rho and the product ONE FP32
 *            multiplication.  (A NaN passes neither comparison.)
 *  Rounds.   The step runs in rounds, at most T of them.  A target's HEAD is the first entry of its list, in list order,
 *            that is admissible and not blocked; an entry is BLOCKED when its squared integer distance di*di + dj*dj to a
 *            position already assigned in this step is below d*d.  Among the heads of the targets not yet assigned the
 *            largest value wins, ties to the smaller t (-0 and +0 tie; a NaN ranks as -inf); the winner is assigned that
 *            position and the round ends.  The step ends when no unassigned target has a head.
 *  Outputs.  An assigned target gets that position and state = the pick's number, 1 ... k.  A target that was never
 *            assigned is HELD: its position stays prev[t], its state is -1.  A held target blocks nobody.
 *  Consequences.  With T = 1 the step is the functor (pick 1, always).  Targets that never come within d of each other's
 *            picks walk exactly the independent chains.  Two targets assigned in one step are never closer than d; only a
 *            held target may be closer than d to another.
 * The rule is defined in LIST ORDER: it does not ask that a list be sorted by value (pdog_detect_peaks sorts picks 2 ... k).
 */
#ifndef PAWSOME_EXCLUSIVE_H
#define PAWSOME_EXCLUSIVE_H

#include "pawsome_peaks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_EXCLUSIVE_MAX_TARGETS 32

/* The rule alone, on DEVICE arrays, for n_groups groups of n_targets targets each: d_prev n_groups x n_targets x 2 int32,
 * d_ij n_groups x n_targets x k x 2 int32, d_peak n_groups x n_targets x k float32, d_count n_groups x n_targets int32 (the
 * outputs of pdog_detect_peaks for the n_groups * n_targets windows, as they lie), d_out_ij n_groups x n_targets x 2 int32,
 * d_out_state n_groups x n_targets int32.  min_distance <= 0 means the default of pawsome_peaks.h, ceil(target_width) with
 * a floor of 1.  One wave per group on the tracker's stream, asynchronous.  PDOG_E_ARG, with nothing launched, for a null
 * pointer, n_groups < 1 (or n_groups * n_targets beyond int32), n_targets outside 1 ... PDOG_EXCLUSIVE_MAX_TARGETS, k
 * outside 1 ... PDOG_PEAKS_MAX_K, min_ratio outside [0, 1] or NaN. */
int pdog_assign_exclusive(pdog_tracker *t, int n_groups, int n_targets, int k, int min_distance, double min_ratio,
                          const int32_t *d_prev, const int32_t *d_ij, const float *d_peak, const int32_t *d_count,
                          int32_t *d_out_ij, int32_t *d_out_state);
/* The same rule in plain C++ on HOST arrays, no GPU and no tracker: min_distance must be given (>= 1).  PDOG_E_ARG,
 * outputs untouched, otherwise as above. */
int pdog_assign_exclusive_host(int n_groups, int n_targets, int k, int min_distance, double min_ratio,
                               const int32_t *prev, const int32_t *ij, const float *peak, const int32_t *count,
                               int32_t *out_ij, int32_t *out_state);

/* The exclusive walk over a frame table: n_groups videos' worth of n_targets targets each on ONE stack of frames.
 * Frames, strides, n_frames, h_table (HOST, n_groups rows of n_steps int32, consumed before the call returns; a group ends
 * where its row turns negative) and `first` as for pdog_detect_chains_indexed (pawsome_video.h) — a row belongs to a GROUP
 * here, all its targets look at the same frame.  d_start is n_groups x n_targets x 2, d_out_ij n_groups x n_targets x
 * n_steps x 2 and d_out_state n_groups x n_targets x n_steps int32 (device).
 *   first = 0: step 0 is the joint step on frame table[g][0] from the starts; step s from out[g][.][s-1], s < len[g]
 *   first = 1: out[g][t][0] = start[g][t] exactly as given, with state 0, when len[g] >= 1; then the same loop for s >= 1
 * state[g][t][s] is the pick's number 1 ... k, or -1 where the target was held.  Steps s >= len[g] are not written.
 * k <= 0 means min(PDOG_PEAKS_MAX_K, 2 * n_targets); min_distance <= 0 the default of pawsome_peaks.h.
 * Per step the call enqueues pdog_detect_peaks for the n_groups * n_targets windows — the maps in the tracker's scratch,
 * whatever batch kernel family the tracker picks for that size, pick 1 under exact mode — and the assignment kernel behind
 * it, both on the tracker's stream, with no host synchronisation between steps.  The table is validated and staged once,
 * before anything is launched.  Asynchronous (the call may wait for the PREVIOUS call's table upload, and drains the stream
 * when a workspace grows); nothing is allocated once sizes repeat.  PDOG_E_ARG, with nothing launched, for everything
 * pdog_assign_exclusive and pdog_detect_chains_indexed refuse (n_groups * n_targets * n_steps beyond int32 included); a
 * device guess out of range arrives through pdog_sync, as for pdog_detect_peaks. */
int pdog_detect_chains_exclusive(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                 int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets,
                                 int first, int k, int min_distance, double min_ratio, const int32_t *d_start,
                                 int32_t *d_out_ij, int32_t *d_out_state);
/* For tests and measurements.  Since the tracker was created: out[0] joint steps enqueued (launches of the assignment
 * kernel), out[1] times a workspace of the two device calls above grew.  No GPU work, no synchronisation. */
int pdog_get_exclusive_counts(pdog_tracker *t, uint64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_EXCLUSIVE_H */
