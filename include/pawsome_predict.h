/*
 * pawsome_predict.h — one-launch chains with a motion model: every clip's window is centred on where its target is PREDICTED
 * to be, and a clip whose window offers nothing coasts and then waits, with state -1, instead of walking to the corner.
 *
 * This is the motion rule of pawsome_motion.h for a group of ONE target with k = 1 — nothing is shared out, nothing is
 * contested, min_distance and min_ratio drop out — served by the kernels that walk a whole clip in one launch (the fused
 * kernel, one workgroup per clip, and the persistent roll chain) instead of two launches per step.  THIS LIBRARY'S ADDITION,
 * like the motion rule; tests/predict_restatement.py states it in NumPy over the dense Float64 oracle, and it equals
 * tests/motion_restatement.py at T = 1, k = 1.  Nothing changes for a caller who does not ask for it.
 *
 * THE RULE — one step of one clip in an h x w frame.
 *  Parameters.  min_response m >= 0, finite, compared as m_f = (float)m; coast >= 0, an int.
 *  State.    The position p filed last (the start, as given, before the first step), the velocity v (two int32) and n_held
 *            (int32).  A walk starts with v = (0, 0) and n_held = 0 unless the caller hands a state in.
 *  1 Prediction.  c = clamp(p + v) into rows 1 ... h and columns 1 ... w (the sum formed without overflow).
 *  2 Window.  The window is centred on c.  R is the FP32 maximum of its response map as the kernel that ran computed it; q is
 *            the functor's clamped position (src/PawsomeTracker.jl:55-62), exact mode's where that is on.
 *  3 Assigned iff R > m_f (a NaN fails): p' = q, state = 1, n_held' = 0, v' = p' - p (modulo 2^32 where that overflows).
 *  4 Held otherwise: state = -1, p' = c, n_held' = n_held + 1 (it stays at INT32_MAX), v' = v while n_held' < coast, (0, 0)
 *            otherwise.  A flat window's response is exactly 0, which does not exceed m = 0.
 *  5 Next guess = clamp(p' + v').
 *  A held frame's position is not used, so the one-launch kernels do not refine a held frame in exact mode: pdog_get_exact's
 *  count of refined windows leaves such frames out, and a lost target does not pay the Float64 refinement on every flat frame.
 *
 * WHICH KERNEL RUNS.  The choice is pdog_detect_chains_indexed's.  Where that is the fused kernel (runtime-length or any
 * compile-time length) or the persistent roll chain (every length with a roll instance), the walk is ONE launch.  The tiled
 * cooperative kernel has no predicted instance: its geometries, the stepped walk's (a table of one step among them) and a
 * kernel length without an instance go to pdog_detect_chains_motion with n_groups = n_clips, n_targets = 1, k = 1 — the same
 * rule by construction, two launches per step.
 */
#ifndef PAWSOME_PREDICT_H
#define PAWSOME_PREDICT_H

#include "pawsome_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The walk over a frame table: pdog_detect_chains_indexed's arguments (pawsome_video.h) with the same meaning and the same
 * validation — one stack of frames, h_table n_clips x n_steps on the host, a clip ends where its row turns negative, `first`
 * — plus min_response, coast, d_out_state and d_mstate.
 *   first = 0: step 0 is the rule on frame table[c][0] from start[c]; step s from what step s - 1 left, s < len[c]
 *   first = 1: out[c][0] = start[c] exactly as given, with state 0, when len[c] >= 1; then the same loop for s >= 1
 * d_out_ij n_clips x n_steps x 2 and d_out_state n_clips x n_steps int32 on the device: state 1 where the clip was assigned,
 * -1 where it was held and out is its prediction.  Steps s >= len[c] are not written.
 * d_mstate n_clips x 4 int32 on the device with the layout of pawsome_motion.h: IN (v_row, v_col, n_held, ignored), OUT the
 * state after each clip's last step, word 3 = 0.  Null: every clip starts at rest and the final state is dropped.  Otherwise
 * a clip's first guess is clamp(start + v), and a walk continued in a second call from the first call's last positions and
 * d_mstate equals the one-call walk.  A clip without a step leaves its d_mstate as it is.
 * Asynchronous on the tracker's stream as pdog_detect_chains_indexed is; nothing is allocated once sizes repeat.
 * PDOG_E_ARG, with nothing launched, for everything pdog_detect_chains_indexed refuses, a min_response that is negative, NaN
 * or infinite, coast < 0, and a null d_out_state. */
int pdog_detect_chains_predicted(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                 int n_frames, const int32_t *h_table, int n_steps, int n_clips, int first,
                                 double min_response, int coast, const int32_t *d_start, int32_t *d_out_ij,
                                 int32_t *d_out_state, int32_t *d_mstate);
/* For tests and measurements.  Since the tracker was created: out[0] launches of the fused kernel's predicted instances,
 * out[1] launches of the persistent chain kernel's, out[2] walks handed to pdog_detect_chains_motion, out[3] times the staged
 * table grew.  No GPU work, no synchronisation. */
int pdog_get_predict_counts(pdog_tracker *t, uint64_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_PREDICT_H */
