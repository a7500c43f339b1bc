/*
 * pawsome_split.h — TOUCHING ANIMALS SPLIT: pawsome_blob.h's measurement with every target's blob restricted to the target's
 * NEAREST-CENTRE CELL among the targets tracked on the same frame.  A header of its own that includes pawsome_blob.h (and with
 * it pawsome_dog.h); neither of them includes this file, and neither changes.
 *
 * This rule lifts the limit pawsome_blob.h ends on: there two animals that touch are one blob, whose orientation, axes and width
 * belong to neither.  Here a pixel belongs to the target whose position is nearest, so the blob of a target stops at the
 * bisector towards its neighbour, and the call says how long the seam is (n_contact).  There is no second fill and there are
 * no competing fronts: the one data-dependent loop is pdog_blob's fill, on a smaller mask, and it ends for the same reason.
 *
 * Positions come in SETS: a set is the n_targets positions (1 ... 32) of the targets on one frame.  THE RULE for target a of a
 * set, in integers up to the twelve sums, exactly.  p = (i, j) is the target's position clamped into the frame as pdog_blob
 * clamps it; frame and radius R are pawsome_shape.h's.
 *   1 - 5a. Patch, lower median b, contrast c, mask and seed are pdog_blob's (pawsome_blob.h), unchanged, every quantity the
 *           target's own.
 *   5c. Cell.   A patch pixel x, in frame coordinates, lies in target a's cell if for EVERY other target b of the same set, q_b
 *               its position clamped into the frame exactly as p is, either |x - p|^2 < |x - q_b|^2, or the two are equal and
 *               a < b.  The arithmetic is integer and exact.  Only the rivals' positions take part: a rival's frame index does
 *               not.  The cells of one set are disjoint in frame coordinates by construction (of two targets at most one wins
 *               a pixel).
 *   5b. Blob.   The connected component of (mask AND cell) that contains the seed, for connectivity 4 or 8.  If the seed is not
 *               in the cell the blob is empty: when a rival with a lower index sits on the same pixel, and when a rival is
 *               within about two pixels and the seed — a pixel of the 3 x 3 — lies on its side.
 *   6. Sums.    Twelve int32 per position: n, Sy, Sx, Syy, Syx, Sxx, b, c, n_mask, n_rim, n_cell, n_contact.  The first ten are
 *               pdog_blob's in its order: the six sums and n_rim taken over THIS blob; b, c and n_mask — the WHOLE mask —
 *               unchanged.  n_cell is the number of mask pixels inside the cell.  n_contact is the number of blob pixels with at
 *               least one of their four EDGE neighbours in (mask AND NOT cell), whatever the connectivity: n_contact > 0 says
 *               that the target touches what lies on a neighbour's side.  An empty blob gives 0 for n, the sums, n_rim and
 *               n_contact.
 *   7. Derived. pdog_shape_derive on the first eight integers, as pdog_blob.
 * CONSEQUENCES.  With n_targets == 1, or with every rival farther than 2R away, the first ten integers are pdog_blob's bit for
 * bit, n_cell == n_mask and n_contact == 0: a patch pixel is at most R from p and then more than R from such a rival.  A rival at
 * distance exactly 2R on an axis still decides one pixel, the tie at distance R from both; so whoever filters rivals keeps
 * those with |p - q|^2 <= (2R)^2.
 */
#ifndef PAWSOME_SPLIT_H
#define PAWSOME_SPLIT_H

#include "pawsome_blob.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_SPLIT_MAX_TARGETS 32

/* The rule for n_sets sets of n_targets positions.  Frames, strides, n_frames, radius, min_contrast, connectivity, asynchrony
 * and stream are pdog_blob's.  Position (s, a) — target a of set s — is element s * set_stride + a * target_stride of d_ij
 * ([.][2] int32, 1-based (row, col)), of d_frame_index (NULL: set s looks at frame s; otherwise int32, one entry per position)
 * and of both outputs, d_out_sums NULL or device [.][12] int32 and d_out_shape NULL or device [.][6] double.  Exactly two
 * layouts are accepted: (set_stride, target_stride) = (n_targets, 1), set-major, and (1, n_sets), target-major — the
 * [n_targets, m] of the chains' results.  PDOG_E_ARG, with nothing launched and a text that names the value, for everything
 * pdog_blob refuses, for n_targets outside 1 ... 32, for any other pair of strides and for n_sets > n_frames without an index.
 * n_sets == 0 does nothing.  Every workgroup ends by itself, as pdog_blob's. */
int pdog_blob_split(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                    const int32_t *d_frame_index, const int32_t *d_ij, int n_sets, int n_targets, int64_t set_stride,
                    int64_t target_stride, int radius, int min_contrast, int connectivity, int32_t *d_out_sums,
                    double *d_out_shape);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_SPLIT_H */
