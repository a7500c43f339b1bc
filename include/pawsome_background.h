/*
 * pawsome_background.h — a STATIC BACKGROUND MODEL: the per-pixel median of some frames of a stack in device memory, and
 * frames with that model subtracted, for the chains to walk instead of the raw grey levels.  Part of the C ABI of
 * pawsome_dog.h, which includes this file at its end (include that one; the types and the status codes are declared
 * there).
 *
 * This is the library's own addition; the reference tracks on the raw frames.  A hole, a stain or a wall edge that is
 * darker than the animal and lies within half a window of its path takes a chain on raw frames for good; it is part of
 * every frame, so it is part of the median, and the subtracted frames do not show it.
 *
 * THE RULE, in integers, exactly.
 *   Model.        For K sample frames, 1 <= K <= PDOG_BG_MAX_SAMPLES, the background pixel is the LOWER MEDIAN of the K
 *                 sample values at that pixel: the value at 0-based rank (K - 1) / 2 (integer division) of the K values
 *                 sorted ascending.  A frame may be named several times; it then counts several times.  A caller may hand
 *                 in an image of their own instead (the empty arena): pdog_bg_set.
 *   Subtraction.  out = clamp(128 + frame - bg, 0, 255) per pixel.  The difference keeps its sign (a darker target stays
 *                 darker than its surroundings, which sit at 128) and saturates at both ends.
 *   Samples.      For a table of m selected frames and a requested K the samples are K' = min(K, m) entries
 *                 table[floor(i * m / K')], i = 0 ... K'-1, in integer arithmetic: pdog_bg_samples.
 */
#ifndef PAWSOME_BACKGROUND_H
#define PAWSOME_BACKGROUND_H

#include "pawsome_dog.h" /* types and status codes (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_BG_MAX_SAMPLES 64

typedef struct pdog_bg pdog_bg; /* opaque: the frame_h x frame_w model of one device, and the staged tables */

/* A handle without a model on HIP device `device`, for frames of frame_h x frame_w.  PDOG_E_ARG for a non-positive size or
 * a device ordinal out of range, PDOG_E_NODEV without a device. */
int pdog_bg_create(int device, int frame_h, int frame_w, pdog_bg **out);
/* Waits for the last stream the handle worked on, then frees it. */
int pdog_bg_destroy(pdog_bg *bg);

/* Host arithmetic, no GPU: the sample rule above.  h_table: m int32 (any values; they are copied, not judged); k: the
 * requested number, 1 ... PDOG_BG_MAX_SAMPLES.  *out_n = min(k, m) always; out_index (may be NULL with cap 0, to ask for
 * the count) receives the samples when cap >= *out_n, and PDOG_E_RANGE is returned otherwise.  PDOG_E_ARG for a null
 * h_table or out_n, m < 1, k outside its range or cap < 0. */
int pdog_bg_samples(const int32_t *h_table, int m, int k, int32_t *out_index, int cap, int *out_n);

/* The model becomes the lower median of the frames h_samples[0 ... n_samples-1] of ONE stack of n_frames frames (device;
 * frame i at d_frames + i*frame_stride, rows row_stride bytes apart; any base address, any row_stride >= frame_w).
 * h_samples is a HOST array, consumed before return; every entry is checked to lie in 0 ... n_frames-1 before anything is
 * launched, so no list can make a kernel read outside the stack.  Nothing outside a row's frame_w bytes is read. */
int pdog_bg_estimate(pdog_bg *bg, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                     int n_frames, const int32_t *h_samples, int n_samples);
/* The model becomes / is copied to a caller's image (device; rows row_stride >= frame_w bytes apart; bytes of d_out
 * between frame_w and row_stride are not written).  pdog_bg_get before any estimate or set is refused. */
int pdog_bg_set(pdog_bg *bg, void *hip_stream, const uint8_t *d_image, int64_t row_stride);
int pdog_bg_get(pdog_bg *bg, void *hip_stream, uint8_t *d_out, int64_t row_stride);

/* out[k] (0 <= k < n_steps; at d_out + k*out_frame_stride, rows out_row_stride bytes apart) is frame h_table[k] of the
 * stack minus the model, by the rule above.  h_table is a HOST array of n_steps int32, consumed before return, and
 * validated as pdog_diag_render_indexed validates its table: every entry in 0 ... n_frames-1, no negative entries; a
 * frame named twice is subtracted twice.  Bytes of d_out between frame_w and out_row_stride are not written.  The outputs
 * must not overlap the stack, the model or each other.  n_steps == 0 does nothing. */
int pdog_bg_subtract_indexed(pdog_bg *bg, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride,
                             int64_t row_stride, int n_frames, const int32_t *h_table, int n_steps, uint8_t *d_out,
                             int64_t out_frame_stride, int64_t out_row_stride);

/* Streams.  Every call but pdog_bg_samples is asynchronous on hip_stream (NULL = the null stream): the model is carried in
 * stream order, and a call on another stream than the last is ordered behind it with the handle's event.  A list or a
 * table goes up on hip_stream through the handle's staging: the host waits only for the PREVIOUS call's words to have left
 * the staging, and drains the stream when their device copy has to grow.
 * Refusals.  PDOG_E_ARG, with nothing launched and the model unchanged, for a null pointer, an entry outside
 * 0 ... n_frames-1, n_samples outside 1 ... PDOG_BG_MAX_SAMPLES, a row stride below frame_w, a negative frame stride,
 * out_frame_stride below (frame_h - 1) * out_row_stride + frame_w with more than one step, a non-positive n_frames, a
 * negative n_steps, and a subtract or get before any estimate or set. */

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_BACKGROUND_H */
