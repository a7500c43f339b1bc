/*
 * pawsome_frame_blobs.h — EVERY CONNECTED BLOB OF A WHOLE FRAME: the connected components of the pixels that depart from a
 * grey level by some contrast, each with its integer moments, labelled on the GPU.  A header of its own that includes
 * pawsome_dog.h (the types and the status codes); pawsome_dog.h does not include this file.
 *
 * This is the library's own addition.  Everything else here is seeded by a known position: the reference's bootstrap looks at
 * a quarter of the frame around its centre (src/PawsomeTracker.jl:99-107), and pdog_shape, pdog_blob and pdog_blob_split
 * measure inside a patch around a position they are given.  This call answers "what is in this frame?".  On a frame with the
 * background removed (pawsome_background.h: everything static sits at 128) "every animal" is every blob that departs from 128.
 *
 * THE RULE, in integers, exactly.
 *   Mask.      A pixel p of the frame is in the mask when level - p >= min_contrast (darker != 0), or p - level >= min_contrast
 *              (darker == 0): its CONTRAST s against `level` reaches min_contrast.  level is 0 ... 255, min_contrast 1 ... 255.
 *              Nothing outside the frame exists: no fill, no patch, no radius.
 *   Blobs.     The connected components of the mask.  connectivity is 4 (two pixels are neighbours if they share an edge) or 8
 *              (an edge or a corner), as in pawsome_blob.h.
 *   Words.     Twelve int64 per blob, rows r and columns c 0-based, in this order:
 *                n, Sy, Sx, Syy, Syx, Sxx   the sums of 1, r, c, r*r, r*c, c*c over the blob's pixels;
 *                rmin, rmax, cmin, cmax     its bounding box;
 *                first                      r * frame_w + c of its first pixel in raster order;
 *                Ss                         the sum of its pixels' contrasts.
 *              The words are 64-bit because the sums need it: Syy of a blob that covers a 3840 x 2160 frame is 1.3e13, far
 *              beyond 32 bits.
 *   Sizes.     The largest words a frame can produce are those of the one blob of a full mask: Syy = w * S2(h),
 *              Sxx = h * S2(w) and Syx = T(h) * T(w), with S2(k) = (k-1)k(2k-1)/6 and T(k) = k(k-1)/2.  A frame size h x w is
 *              ADMITTED when all of these hold, so that no word of an admitted frame leaves 63 bits:
 *                h >= 1 and w >= 1;   h * w <= 2^30;   w <= PDOG_MAX_ROW_STRIDE (a call's row_stride is at least w);
 *                w * S2(h) <= 2^63 - 1;   h * S2(w) <= 2^63 - 1;   T(h) * T(w) <= 2^63 - 1.
 *              The largest h admitted, by width:
 *                w          1          2          64       1920     3840     16 384   32 768   2^21
 *                h      3 024 617  2 400 640   756 154   243 353  193 149   65 536   32 768     3
 *              (at w = 16 384 and 32 768 the pixel limit binds first).  pdog_fb_create refuses every other size: beyond these
 *              the 64-bit atomics would wrap modulo 2^64 without a sign, and the derived values would be garbage.
 *   Filter.   The blobs with min_area <= n <= max_area are KEPT.
 *   Order.     Kept blobs are listed in ascending `first` — the order in which scipy.ndimage.label numbers components.  It is a
 *              property of the frame alone, so the result does not depend on how the kernels are scheduled.
 *   Count.     Per step, count = the number of kept blobs and n_mask = the number of mask pixels.  At most `cap` blobs are
 *              written, the first `cap` in that order; count > cap says that the list is cut.  Rows of the output behind
 *              min(count, cap) are zero.
 *   Derived.   pdog_frame_blobs_derive turns a blob's twelve words into six Float64: row and column of the centroid, 1-BASED
 *              like every position of this library (1 + Sy / n, 1 + Sx / n), then theta, major axis, minor axis and equivalent
 *              width by pawsome_shape.h's step 7.  The central second moments' numerators n*Syy - Sy*Sy, n*Sxx - Sx*Sx and
 *              n*Syx - Sy*Sx are formed in exact 128-bit integer arithmetic before the first floating-point operation.
 *
 * HOW IT ENDS.  Labels are pixel indices r * frame_w + c, and a blob's label is its smallest one: `first`.  The kernels join
 * labels with a union-find whose only write is an atomic minimum on the parent of the larger of two roots.  No kernel waits
 * for another workgroup: there is no spin, no flag and no cooperative launch.  Every loop either LOWERS A LABEL OR ENDS:
 *   find(x)      reads x's parent y; y == x ends the loop, otherwise y < x and the loop goes on from y (having hung x under y's
 *                parent, an atomic minimum too: path splitting).  Parents only ever decrease and never fall below 0, so it ends
 *                whatever other workgroups do meanwhile.
 *   union(a, b)  finds both roots; equal roots end the loop.  Otherwise the atomic minimum writes the smaller root into the
 *                larger root's parent and returns what stood there: the larger root itself ends the loop (it was a root, and is
 *                joined now); anything else is a label BELOW the larger root, from which the loop goes on.
 * All sums are integer atomics, so the result does not depend on their order; nothing of this rule is accumulated in floating
 * point on the device.
 */
#ifndef PAWSOME_FRAME_BLOBS_H
#define PAWSOME_FRAME_BLOBS_H

#include "pawsome_dog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_FB_WORDS 12           /* int64 per blob */
#define PDOG_FB_MAX_IN_FLIGHT 1024 /* steps a handle may hold scratch for */

typedef struct pdog_fb pdog_fb; /* opaque: the label and area scratch of one device for steps_in_flight frames, the staged table */

/* A handle on HIP device `device` for frames of frame_h x frame_w (an admitted size: "Sizes" above) that labels up to
 * steps_in_flight frames (1 ... PDOG_FB_MAX_IN_FLIGHT) per round of kernels; it owns 8 bytes of scratch per pixel and step in
 * flight.  PDOG_E_ARG for a size that is not admitted (before any device is asked for; the text names the size and the word
 * that would not fit), a number outside its range or a device ordinal out of range, PDOG_E_NODEV without a device,
 * PDOG_E_ALLOC when the scratch does not fit. */
int pdog_fb_create(int device, int frame_h, int frame_w, int steps_in_flight, pdog_fb **out);
/* Waits for the last stream the handle worked on, then frees it. */
int pdog_fb_destroy(pdog_fb *fb);

/* The rule for the frames h_table[0 ... n_steps-1] of ONE stack of n_frames frames (device; frame i at
 * d_frames + i*frame_stride, rows row_stride bytes apart; any base address, any row_stride >= frame_w, as
 * pdog_bg_subtract_indexed takes them).  h_table is a HOST array, consumed before return; every entry is checked to lie in
 * 0 ... n_frames-1 before anything is launched, and a frame may be named twice.  Nothing outside a row's frame_w bytes is read.
 * d_out_words: device [n_steps][cap][12] int64, d_out_count: device [n_steps][2] int32 (count, n_mask); both are written whole.
 * Steps beyond the handle's steps_in_flight are processed in rounds inside this one call.  n_steps == 0 does nothing.
 * Asynchronous on hip_stream (NULL = the null stream) and ordered as pawsome_background.h describes: a call on another stream
 * than the last is ordered behind it with the handle's event, and the table goes up through the handle's staging.
 * Refusals.  PDOG_E_ARG, with nothing launched and nothing written, for a null pointer, a table entry outside the stack,
 * level outside 0 ... 255, min_contrast outside 1 ... 255, a connectivity other than 4 or 8, min_area < 1, max_area < min_area,
 * cap < 1, a row stride below frame_w or above PDOG_MAX_ROW_STRIDE, a negative frame stride, a non-positive n_frames and a
 * negative n_steps.  The error text names the offending value. */
int pdog_frame_blobs(pdog_fb *fb, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                     int n_frames, const int32_t *h_table, int n_steps, int level, int darker, int min_contrast,
                     int connectivity, int64_t min_area, int64_t max_area, int cap, int64_t *d_out_words, int32_t *d_out_count);

/* Host arithmetic, no GPU: the rule's derived values of one blob.  out = {row, col, theta, major, minor, width}, all NaN
 * for n <= 0.  PDOG_E_ARG for a null pointer. */
int pdog_frame_blobs_derive(const int64_t words[12], double out[6]);

/* THE STARTS OF track_video(find="frame") are this library's choice, stated here because they are built on this rule: on the
 * first frame the tracker sees, with level 128 under `background` and the frame's mode otherwise, the blobs with
 * max(1, W*W/5) <= n <= 3*W*W, W = ceil(target_width) — a quarter to about four times a disc of the target's width — are kept,
 * the K of largest n are taken (ties to the lower `first`; target 0 is the largest), and their centroids, rounded half to
 * even, are the guesses that the tracker's own detection refines. */

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_FRAME_BLOBS_H */
