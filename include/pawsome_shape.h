/*
 * pawsome_shape.h — HOW A TARGET LIES at a tracked position: the orientation of its body axis, its two axes and its width,
 * measured on the frame around the position.  Part of the C ABI of pawsome_dog.h, which includes this file at its end
 * (include that one; the types and the status codes are declared there).
 *
 * This is the library's own addition; the reference returns positions and nothing like this.  What a tracker's user asks
 * for right after the track is the heading, the elongation (is this still my animal, two merged animals, or nothing?) and
 * the width to hand over as target_width.
 *
 * THE RULE, in integers up to the eight sums, exactly.  A position (i, j) is 1-based (row, col) and is clamped into the
 * frame first, as pdog_measure clamps it.  It is measured on ONE frame with a radius R, 2 <= R <= PDOG_SHAPE_MAX_RADIUS.
 *   1. Patch.      The pixels at offsets (dy, dx), dy*dy + dx*dx <= R*R, around the position.  A pixel outside the frame has
 *                  the tracker's fill value (the PaddedView rule, src/PawsomeTracker.jl:48).  N, the number of patch pixels,
 *                  depends on R only.
 *   2. Background. b = the LOWER MEDIAN of the N patch values: the value at 0-based rank (N - 1) / 2 (integer division) of
 *                  the values sorted ascending — the convention of pawsome_background.h.
 *   3. Contrast.   s(p) = b - p for a darker_target tracker, p - b otherwise.
 *   4. Target.     c = max(0, max of s over the 3 x 3 pixels around the position), fill outside the frame.
 *   5. Mask.       Empty if c < min_contrast.  Otherwise the patch pixels with 2 * s(p) >= c: at or above half the target's
 *                  own contrast.
 *   6. Sums.       Eight int32 per position, in this order: n, Sy, Sx, Syy, Syx, Sxx, b, c — the mask's pixel count and the
 *                  sums of dy, dx, dy*dy, dy*dx, dx*dx over the mask.  With R <= 127 every sum stays below 2^31: the sum of
 *                  dy*dy + dx*dx over the WHOLE disc is about pi R^4 / 2 = 4.1e8, and no other sum exceeds it.
 *   7. Derived.    Six Float64 per position: row, col, theta, major, minor, width.  n == 0 makes all six NaN.  Otherwise,
 *                  with the exact int64 numerators A = n*Syy - Sy*Sy, B = n*Sxx - Sx*Sx, C = n*Syx - Sy*Sx:
 *                    myy = A/n^2 + 1/12, mxx = B/n^2 + 1/12, myx = C/n^2        (a pixel is a unit square)
 *                    row = i + Sy/n, col = j + Sx/n
 *                    theta = 0.5 * atan2(2 myx, mxx - myy)     the MAJOR axis, measured from +col towards +row, in
 *                                                              (-pi/2, pi/2]; 0 for an isotropic mask
 *                    t = hypot(2 myx, mxx - myy)
 *                    major = 4 sqrt((mxx + myy + t) / 2), minor = 4 sqrt(max((mxx + myy - t) / 2, 0))
 *                                                              the FULL axes of the uniform ellipse with those moments
 *                    width = 2 sqrt(n / pi)                    the equivalent diameter: the number to use as target_width
 *                  Every operation is rounded on its own (no contraction).  sqrt and the four basic operations are
 *                  correctly rounded everywhere; atan2 and hypot are the math library's, so theta, major and minor of the
 *                  host and of the device may differ in their last bits.
 *   8. Heading.    Host only, a sequential rule per target over its steps; it resolves theta's 180 degree ambiguity with
 *                  the motion.  For step k take d = ij[k] - ij[k-1].  If k >= 1 and |d|^2 >= min_step^2: of theta and
 *                  theta + pi the one whose direction (d_row, d_col) = (sin, cos) has a non-negative dot product with d
 *                  (zero takes theta).  Otherwise the one within pi/2 of the previous heading (a tie takes theta); with no
 *                  previous heading, theta itself.  A NaN theta gives a NaN heading and leaves the previous heading as it
 *                  was.  The result is wrapped to (-pi, pi].
 *
 * KNOWN LIMIT.  The mask is not restricted to the connected blob under the position: a second object inside the patch that
 * reaches half the target's contrast is counted.  A background model (pawsome_background.h) and a radius that fits the
 * animal are the remedies; connected-component labelling is not part of this rule.
 */
#ifndef PAWSOME_SHAPE_H
#define PAWSOME_SHAPE_H

#include "pawsome_dog.h" /* types and status codes (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_SHAPE_MAX_RADIUS 127

/* The rule's steps 1 - 7 for n positions.  Arguments and refusals are pdog_measure's: position b (d_ij: device, [n][2]
 * int32) looks at frame d_frame_index[b] (device, int32; NULL: frame b) of the stack d_frames (frame k at
 * d_frames + k*frame_stride, rows row_stride bytes apart; any base address, any row_stride >= frame_w; nothing outside a
 * row's frame_w bytes is read).  radius: 0 = the default, ceil(target_width) of the tracker capped at
 * PDOG_SHAPE_MAX_RADIUS (and at least 2), or 2 ... PDOG_SHAPE_MAX_RADIUS; min_contrast: 1 ... 255.  d_out_sums: NULL or
 * device [n][8] int32; d_out_shape: NULL or device [n][6] double.  Asynchronous on the tracker's stream.  Reads the
 * tracker's frame size, fill, darker_target and target_width and nothing else.
 * PDOG_E_ARG, with nothing launched, for a null tracker, null frames or positions, both outputs NULL, n < 0,
 * n_frames <= 0, a row stride below frame_w or above PDOG_MAX_ROW_STRIDE, a negative frame stride, more positions than
 * frames without an index, a radius outside {0} and 2 ... 127 and a min_contrast outside 1 ... 255.  n == 0 does nothing. */
int pdog_shape(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
               const int32_t *d_frame_index, const int32_t *d_ij, int n, int radius, int min_contrast,
               int32_t *d_out_sums, double *d_out_shape);

/* Host arithmetic, no GPU: step 7 for one position.  ij is clamped by nobody here: it is the CLAMPED position the sums were
 * taken at.  PDOG_E_ARG for a null pointer. */
int pdog_shape_derive(const int32_t sums[8], const int32_t ij[2], double out[6]);

/* Host arithmetic, no GPU: step 8 for one target.  theta: n_steps doubles; ij: [n_steps][2] int32; out: n_steps doubles.
 * PDOG_E_ARG for a null pointer, n_steps < 0 and a min_step that is negative or NaN.  n_steps == 0 does nothing. */
int pdog_shape_headings(const double *theta, const int32_t *ij, int n_steps, double min_step, double *out);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_SHAPE_H */
