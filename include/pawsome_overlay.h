/*
 * pawsome_overlay.h — the diagnostic overlay over a FRAME TABLE and for SEVERAL TARGETS: what the chains over a frame
 * table (pawsome_video.h) return, drawn without gathering the selected frames into a second stack.  Part of the C ABI of
 * pawsome_dog.h, which includes this file at its end (include that one; the types, the status codes and the overlay's
 * handle are declared there).
 *
 * The reference's public call is track(file; start, stop, fps, ..., diagnostic_file) (src/PawsomeTracker.jl:130-146); its
 * overlay video (src/diagnose.jl) is drawn from the frames ffmpeg selected.  Here the selection is a table of frame
 * indices into a stack in device memory, and the renderer walks that table as the chains do.  The reference has one
 * target per video; several targets on one overlay are this library's addition: every target has its own trace, all are
 * drawn in the handle's colour onto the same buffers.
 */
#ifndef PAWSOME_OVERLAY_H
#define PAWSOME_OVERLAY_H

#include "pawsome_dog.h" /* types, status codes and pdog_diag (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_DIAG_MAX_TARGETS 1024

/* Number of traces the handle carries (1 after pdog_diag_create).  Empties every trace, also when n is the
 * current number.  Ordered on the handle's last stream like a render (the host waits for that stream only where the
 * trace state has to grow).  PDOG_E_ARG for n outside 1 ... PDOG_DIAG_MAX_TARGETS.  Should the allocation of a larger state
 * fail (PDOG_E_HIP), the handle carries no trace (0 targets) and refuses every render until a later call succeeds.
 * On a handle set to more than one target the contiguous render of pawsome_dog.h returns PDOG_E_ARG, with nothing
 * launched and the traces unchanged: it takes one row of positions.  That is the only new behaviour of that call. */
int pdog_diag_set_targets(pdog_diag *d, int n_targets);
int pdog_diag_get_targets(const pdog_diag *d, int *out_n_targets);

/* Output k (0 <= k < n_steps) is frame h_table[k] of ONE stack of n_frames frames, resized as pdog_diag_render
 * resizes it.  For every target t it carries the dot at target t's position of step k and the path of target t's
 * last <= 100 scaled points (the handle's earlier ones, then steps 0 ... k of this call), all in the handle's colour.
 * Target t's position of step k is the int32 pair at d_ij + 2*(t*ij_target_stride + k) (device; ij_target_stride in
 * positions, >= n_steps), so a column slice out[:, k0:k1] of a chains result is passed as it lies.
 * h_table is a HOST array of n_steps int32, consumed before return.
 * d_out is n_steps x 360 x 640, contiguous.
 *
 * Validation.  The table is checked before anything is queued: every entry lies in 0 ... n_frames-1.  No negative
 * entries are allowed (a shorter clip is a smaller n_steps), and a frame named twice is resized twice.  No table can
 * therefore make a kernel read outside the stack.
 * A refused call changes nothing: PDOG_E_ARG, with nothing launched and the traces unchanged, for a bad table entry,
 * n_targets different from the handle's number of targets, ij_target_stride < n_steps, a null pointer, a non-positive
 * frame size or n_frames, row_stride < frame_w, or a negative frame_stride or n_steps.  n_steps == 0 does nothing.
 * Equivalence.  With one target and the table 0 ... n-1 the output equals pdog_diag_render's, byte for byte, and a
 * handle's trace may pass between the two calls in either order.
 * Streams.  As for pdog_diag_render: asynchronous on hip_stream, no host wait for the device, the traces carried in
 * stream order, and a call on another stream than the last ordered behind it with the handle's event.  The table goes
 * up on hip_stream through the handle's staging: the host waits only for the PREVIOUS call's table to have left the
 * staging, and drains the stream when the device copy of the table has to grow.  pdog_diag_destroy drains the last
 * stream before anything is freed.
 * Drawing order.  Positions are clamped into the frame before scaling.  All stores are of one colour, so the targets
 * need no order among themselves. */
int pdog_diag_render_indexed(pdog_diag *d, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride,
                             int64_t row_stride, int frame_h, int frame_w, int n_frames, const int32_t *h_table,
                             int n_steps, const int32_t *d_ij, int64_t ij_target_stride, int n_targets,
                             uint8_t *d_out);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_OVERLAY_H */
