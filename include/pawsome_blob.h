/*
 * pawsome_blob.h — THE SHAPE OF THE CONNECTED BLOB under a tracked position: pawsome_shape.h's measurement with the mask
 * restricted to the connected component the position lies on.  A header of its own that includes pawsome_dog.h (and with it
 * pawsome_shape.h); pawsome_dog.h does not include this file.
 *
 * This rule lifts the KNOWN LIMIT of pawsome_shape.h: there a second object inside the patch that reaches half the target's
 * contrast is counted with the target; here it is not, and the call says that it was there (n_mask > n).  What this rule
 * does NOT do: two animals that TOUCH are still one blob.  major / minor, and n against the expected area, are how a caller
 * sees that.
 *
 * THE RULE, in integers up to the ten sums, exactly.  Position, frame and radius R are pawsome_shape.h's.
 *   1. Patch.      The pixels at offsets (dy, dx), dy*dy + dx*dx <= R*R, around the position.  A pixel outside the frame has
 *                  the tracker's fill value (the PaddedView rule, src/PawsomeTracker.jl:48).  N, the number of patch pixels,
 *                  depends on R only.
 *   2. Background. b = the LOWER MEDIAN of the N patch values: the value at 0-based rank (N - 1) / 2 (integer division) of
 *                  the values sorted ascending — the convention of pawsome_background.h.
 *   3. Contrast.   s(p) = b - p for a darker_target tracker, p - b otherwise.
 *   4. Target.     c = max(0, max of s over the 3 x 3 pixels around the position), fill outside the frame.
 *   5. Mask.       Empty if c < min_contrast.  Otherwise the patch pixels with 2 * s(p) >= c: at or above half the target's
 *                  own contrast.
 *   5a. Seed.      The first pixel of the 3 x 3 around the position, in row-major order (dy ascending, then dx ascending),
 *                  whose s equals c.  It lies inside the disc because R >= 2 and inside the mask because c >= 1 there
 *                  (2 c >= c).
 *   5b. Blob.      The connected component of the mask that contains the seed.  connectivity is 4 (two pixels are neighbours
 *                  if they share an edge) or 8 (an edge or a corner).  Pixels outside the frame carry the fill and take part
 *                  like any other pixel; pixels outside the disc are never in the mask, so the blob never leaves the disc.
 *   6. Sums.       Ten int32 per position, in this order: n, Sy, Sx, Syy, Syx, Sxx, b, c, n_mask, n_rim.  The first six are
 *                  pawsome_shape.h's sums taken over the BLOB; b and c are as there.  n_mask is the pixel count of the whole
 *                  mask — pdog_shape's n —, so n_mask > n says that something else in the patch reaches half the target's
 *                  contrast.  n_rim is the number of blob pixels with at least one of their four EDGE neighbours outside the
 *                  disc, whatever the connectivity: n_rim > 0 says that the blob is cut by the patch — the radius is too
 *                  small or the object larger than thought.  An empty mask gives 0, 0, 0, 0, 0, 0, b, c, 0, 0.
 *   7. Derived.    pdog_shape_derive on the first eight integers: six Float64 per position, row, col, theta, major, minor,
 *                  width, all NaN for an empty mask.  There is no arithmetic of this rule's own in Float64.
 * Where the mask is one component, the first eight integers are pdog_shape's, bit for bit.
 */
#ifndef PAWSOME_BLOB_H
#define PAWSOME_BLOB_H

#include "pawsome_dog.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule's steps 1 - 7 for n positions.  Arguments, asynchrony and refusals are pdog_shape's (pawsome_shape.h), with
 * connectivity, 4 or 8, in addition, d_out_sums NULL or device [n][10] int32 and d_out_shape NULL or device [n][6] double.
 * PDOG_E_ARG, with nothing launched, for everything pdog_shape refuses and for a connectivity other than 4 or 8 (the error
 * text names the value).  n == 0 does nothing.  Every workgroup ends by itself: the fill waits for no other workgroup, and
 * each of its sweeps either adds a pixel to the blob or is the last. */
int pdog_blob(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
              const int32_t *d_frame_index, const int32_t *d_ij, int n, int radius, int min_contrast, int connectivity,
              int32_t *d_out_sums, double *d_out_shape);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_BLOB_H */
