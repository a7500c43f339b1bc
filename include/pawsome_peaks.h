/*
 * pawsome_peaks.h — several targets in one window: the K best, mutually separated peaks of a window's DoG response.
 *
 * The reference finds ONE target per window: `findmax` over the response (src/PawsomeTracker.jl:59), and its only
 * bootstrap is that findmax over the sz .÷ 4 window (:99-107).  The selection below is THIS LIBRARY'S ADDITION, like the
 * sub-pixel rule and several targets per video; tests/peaks_restatement.py states it in NumPy and the kernel
 * (csrc/dog_peaks.hpp) is held to that statement bit for bit.
 *
 * THE RULE, for one window with guess g, radii r and an H x W frame:
 *  Map.     R is the FP32 response map the kernel family that ran writes for the window (d_out_resp of pdog_detect_batch):
 *           column-major, window pixel (row, col) — frame pixel (g1 - r1 + row, g2 - r2 + col), rows and columns of the
 *           window counted from 0 — at idx = col * win_h + row.
 *  Pick 1   is the position pdog_detect_batch returns for the window, always: exact mode on, off or 2, clamped to the frame
 *           (:61).  Its reported value is the maximum of R over the whole window, NaNs left out (the value at the first idx
 *           that holds it; -inf for a window of NaNs).
 *  Candidates for picks 2 ... K are the window pixels p that
 *           (a) lie inside the frame,
 *           (b) are a local maximum of R among their up to eight neighbours that lie in the window: R(p) > R(q) for a
 *               neighbour q with a smaller idx, R(p) >= R(q) for one with a larger idx (a tied pair has exactly one local
 *               maximum, the column-major first; a comparison with a NaN neighbour fails), and
 *           (c) hold no NaN.
 *  Greedy selection.  Pick k is the candidate with the largest R, ties to the smallest idx, among the candidates not
 *           suppressed; a candidate is suppressed when its squared distance di*di + dj*dj (integers, frame coordinates) to
 *           ANY earlier pick — pick 1 included, at its clamped position — is below min_distance * min_distance.  The
 *           selection ends when no candidate is left or K picks are made.
 *  Outputs per window: count in 1 ... K; count 1-based (row, col) positions and FP32 values in pick order; the entries
 *           beyond count are (0, 0) and -inf.
 *  min_distance <= 0 means the default, ceil(target_width), with a floor of 1.
 *
 * SCOPE OF THE GUARANTEE.  Exact mode (pawsome_dog.h) makes pick 1 the position of this repository's restatement of the
 * reference, under the two last-bit assumptions named there (Float64(::N0f8) is pixel / 255.0; ImageFiltering's FIR inner
 * loop is a sequential `tmp += a*b`).  Picks 2 ... K are ranked in FP32, on the map of whichever kernel family ran: they
 * are the library's own addition, exact mode does not re-decide them, and two candidates whose Float64 responses differ by
 * less than that family's FP32 error (delta, pawsome_dog.h) may come out in either order.
 */
#ifndef PAWSOME_PEAKS_H
#define PAWSOME_PEAKS_H

#include "pawsome_dog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_PEAKS_MAX_K 32

/* The K best separated peaks of n windows.  Arguments as for pdog_detect_batch (all pointers DEVICE pointers); further
 *  k            picks per window, 1 ... PDOG_PEAKS_MAX_K
 *  min_distance see above
 *  d_out_ij     n x k x 2 int32
 *  d_out_peak   NULL, or n x k float32
 *  d_out_count  NULL, or n int32
 *  d_out_resp   NULL, or n x win_h x win_w float32: the maps the picks were taken from.  Without it the maps go to scratch
 *               of the tracker's, at most PDOG_MAP_MB of it (never less than one window's), and the windows are served in
 *               chunks that fit: no batch size is an error.
 * The tracker's normal batch path runs with the map (the kernel family pdog_kernel_for_batch names for the chunk's size)
 * and the selection kernel behind it, one workgroup per window, on the tracker's stream.  Asynchronous like
 * pdog_detect_batch; a device guess out of range is reported by pdog_sync as for that call (the picks of such a window are
 * then taken over the fill value's response).  PDOG_E_ARG, before anything is launched, for a null tracker, null frames,
 * guesses or d_out_ij, k outside 1 ... PDOG_PEAKS_MAX_K, n < 0, and the stride and frame errors of pdog_detect_batch;
 * n == 0 does nothing.
 * pdog_set_tuning key "peaks_no_list" (0 / 1): the selection rounds scan the map itself instead of the candidate list the
 * kernel keeps in LDS — the path a window with more candidates than the list holds takes by itself; same picks, slower. */
int pdog_detect_peaks(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                      int n_frames, const int32_t *d_frame_index, const int32_t *d_guesses, int n,
                      int k, int min_distance, int32_t *d_out_ij, float *d_out_peak,
                      int32_t *d_out_count, float *d_out_resp);
/* For tests and measurements.  Since the tracker was created: out[0] windows the selection kernel served, out[1] those
 * among them whose candidates overflowed the list (their rounds scanned the map).  Drains the stream and reports what its
 * kernels raised, like pdog_sync. */
int pdog_get_peaks_counts(pdog_tracker *t, uint64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_PEAKS_H */
