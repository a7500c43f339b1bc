/*
 * pawsome_motion.h — exclusive chains with a motion model: every target's window is centred on where the target is PREDICTED
 * to be, the targets share out the peaks by nearness to their predictions, and a target that finds nothing coasts.
 *
 * The exclusive step (pawsome_exclusive.h) centres each window on the previous position and hands out peaks by value.  Two
 * equal targets that cross may therefore swap identities on a last-bit tie, the window has to be as large as the target is
 * fast, and a target whose window goes flat walks off to the window's first pixel without a word.  The step below is THIS
 * LIBRARY'S ADDITION, like the exclusive rule and the K-peaks selection it builds on; tests/motion_restatement.py states it
 * in NumPy, and the kernel (csrc/dog_motion.hpp) and the host function are held to that statement bit for bit.  Nothing
 * changes for a caller who does not ask for it.
 *
 * THE RULE — one joint step for one GROUP of T targets in an h x w frame, T <= PDOG_MOTION_MAX_TARGETS.
 *  Parameters.  k and min_distance d >= 1 as for the exclusive step; min_ratio rho in [0, 1], rho_f = (float)rho;
 *            min_response m >= 0, finite, compared as m_f = (float)m; coast c >= 0, an int.
 *  State.    Per target its position p, its velocity v (two int32) and n_held (int32), carried from step to step.  A walk
 *            starts with v = (0, 0) and n_held = 0.
 *  1 Prediction.  c_t = clamp(p_t + v_t) into rows 1 ... h and columns 1 ... w (the sum formed without overflow).  The
 *            target's window is centred on c_t, not on p_t: its list ij[t][0 .. k-1], peak[t][0 .. k-1], count[t] is
 *            pdog_detect_peaks at guess c_t.
 *  2 Admissible.  Entry q is admissible iff (q = 0 or q < count[t]) and peak[t][q] > m_f and peak[t][q] >= rho_f * peak[t][0],
 *            the product ONE FP32 multiplication.  A NaN passes nothing.  Pick 1 is NOT exempt, unlike the exclusive rule: a
 *            flat or empty window offers nothing, which is what lets a lost target be noticed.
 *  3 Distance.  D(t, q) is the squared integer distance from ij[t][q] to c_t as an unsigned 32-bit number: 0xFFFFFFFF when
 *            either |difference| is 65536 or more, min(di*di + dj*dj, 0xFFFFFFFF) otherwise — defined for any int32 input.
 *  4 Head.   The head of an unassigned target is its entry of smallest D among those admissible and not blocked, ties to the
 *            smaller q.  BLOCKED as in pawsome_exclusive.h: the squared integer distance to a position assigned in this step is
 *            below d*d.
 *  5 Round.  At most T rounds.  Among the heads of the unassigned targets the smallest D wins, ties to the larger value (-0
 *            and +0 tie, a NaN ranks as -inf), then to the smaller t; the winner takes that position.  The step ends when no
 *            unassigned target has a head.
 *  6 Assigned.  p' = the pick, state = the pick's number 1 ... k, n_held' = 0.  The target is CONTESTED when p' lies within d
 *            of another target's prediction c_u — squared distance below d*d, u != t, u assigned or not.  A contested target
 *            keeps its velocity, v' = v: a blob shared with another target says nothing about this target's own motion.
 *            Otherwise v' = p' - p_t (modulo 2^32 where that overflows).
 *  7 Held (never assigned).  state = -1, n_held' = n_held + 1 (it stays at INT32_MAX), p' = c_t: the target coasts.
 *            v' = v while n_held' < c, (0, 0) otherwise.  A held target blocks nobody.
 *  8 Next guess = clamp(p' + v').
 *  Consequences.  A target that never moves walks its independent chain exactly (as long as its responses pass m and nothing
 *            comes within d).  Two targets assigned in one step are never closer than d.  With coast = 3 a target whose disc
 *            vanishes is held from that step on: it advances by v on three steps and then stays where it is, state -1
 *            throughout.  (coast = 0 and coast = 1 are the same: the step that first holds a target files the prediction,
 *            which has already advanced by v once.)
 * The rule is defined over the lists as they lie; it does not ask that they be sorted.
 */
#ifndef PAWSOME_MOTION_H
#define PAWSOME_MOTION_H

#include "pawsome_exclusive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_MOTION_MAX_TARGETS 32

/* The rule alone, on DEVICE arrays, for n_groups groups of n_targets targets each; h and w are the tracker's frame size.
 * d_prev n_groups x n_targets x 2 int32, the positions p; d_mstate n_groups x n_targets x 4 int32, IN (v_row, v_col, n_held,
 * ignored) and OUT (v', n_held', 0); d_ij, d_peak, d_count the outputs of pdog_detect_peaks for the n_groups * n_targets
 * windows at the PREDICTIONS clamp(p + v), as they lie (pawsome_exclusive.h gives the shapes); d_out_ij n_groups x n_targets
 * x 2, the positions p'; d_out_state n_groups x n_targets; d_next n_groups x n_targets x 2, the next guesses.  d_out_ij and
 * d_next may each be d_prev.  min_distance <= 0 means the default of pawsome_peaks.h.  One wave per group on the tracker's
 * stream, asynchronous.  PDOG_E_ARG, with nothing launched, for everything pdog_assign_exclusive refuses, a min_response
 * that is negative, NaN or infinite, and coast < 0. */
int pdog_assign_motion(pdog_tracker *t, int n_groups, int n_targets, int k, int min_distance, double min_ratio,
                       double min_response, int coast, const int32_t *d_prev, int32_t *d_mstate, const int32_t *d_ij,
                       const float *d_peak, const int32_t *d_count, int32_t *d_out_ij, int32_t *d_out_state, int32_t *d_next);
/* The same rule in plain C++ on HOST arrays, no GPU and no tracker: min_distance must be given (>= 1), and so must the
 * frame size, frame_h and frame_w >= 1.  PDOG_E_ARG, outputs and mstate untouched, otherwise as above. */
int pdog_assign_motion_host(int n_groups, int n_targets, int k, int min_distance, double min_ratio, double min_response,
                            int coast, int frame_h, int frame_w, const int32_t *prev, int32_t *mstate, const int32_t *ij,
                            const float *peak, const int32_t *count, int32_t *out_ij, int32_t *out_state, int32_t *next);

/* The walk over a frame table: pdog_detect_chains_exclusive's arguments (pawsome_exclusive.h) with the same meaning — frames,
 * strides, h_table, `first`, k <= 0 and min_distance <= 0 for the defaults — plus min_response, coast and d_mstate, n_groups
 * x n_targets x 4 int32 on the device as above.  A null d_mstate means the walk starts at rest and its final state is
 * dropped.  Otherwise the walk starts from that state — the first guess of a target is clamp(start + v) — and d_mstate holds
 * the state after each group's last step when the call's work is done: a walk continued in a second call from the first
 * call's last positions and d_mstate equals the one-call walk.
 *   first = 0: step 0 is the joint step on frame table[g][0] from the starts; step s from out[g][.][s-1], s < len[g]
 *   first = 1: out[g][t][0] = start[g][t] exactly as given, with state 0, when len[g] >= 1; then the same loop for s >= 1
 * state[g][t][s] is the pick's number 1 ... k, or -1 where the target was held and out[g][t][s] is its prediction.  Steps
 * s >= len[g] are not written, and a group without a step leaves its d_mstate as it is.
 * Per step the call enqueues pdog_detect_peaks for the n_groups * n_targets windows at the predictions and the motion kernel
 * behind it, both on the tracker's stream, with no host synchronisation between steps.  The table is validated and staged
 * once, before anything is launched.  Asynchronous as pdog_detect_chains_exclusive is; nothing is allocated once sizes
 * repeat.  PDOG_E_ARG, with nothing launched, for everything pdog_assign_motion and pdog_detect_chains_exclusive refuse. */
int pdog_detect_chains_motion(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                              int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets, int first,
                              int k, int min_distance, double min_ratio, double min_response, int coast,
                              const int32_t *d_start, int32_t *d_out_ij, int32_t *d_out_state, int32_t *d_mstate);
/* For tests and measurements.  Since the tracker was created: out[0] motion steps enqueued (launches of the motion kernel),
 * out[1] times a workspace of the two device calls above grew.  No GPU work, no synchronisation. */
int pdog_get_motion_counts(pdog_tracker *t, uint64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_MOTION_H */
