"""NumPy restatement of the split rule (include/pawsome_split.h): steps 1 - 5a as tests/blob_restatement.py has them, the cell by
the PER-PIXEL inequality against every other position of the set (integers; no row intervals), blob_restatement.flood on
mask AND cell, the twelve integers in int64, and shape_restatement.derive on the first eight.  Written from the header's text,
not from the library's code.  TEST HELPER: nothing here loads the library under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blob_restatement as BLR  # noqa: E402
from shape_restatement import derive  # noqa: E402


def clamp(ij, h, w):
    return min(max(int(ij[0]), 1), h), min(max(int(ij[1]), 1), w)


def cell_at(p, a, positions, R, h, w):
    """Step 5c for target `a` of a set: bool [D, D] over the bounding box of the patch around the clamped position p.  positions:
    the set's positions as given (clamped here, as p was)."""
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    y, x = (p[0] + dy).astype(np.int64), (p[1] + dx).astype(np.int64)       # frame coordinates, 1-based like the positions
    own = (y - p[0]) ** 2 + (x - p[1]) ** 2
    cell = np.ones(own.shape, bool)
    for b, q in enumerate(positions):
        if b == a:
            continue
        q = clamp(q, h, w)
        other = (y - q[0]) ** 2 + (x - q[1]) ** 2
        cell &= (own < other) | ((own == other) & (a < b))
    return cell


def parts_at(frame, positions, a, R, fill, darker, min_contrast, connectivity):
    """Steps 1 - 5b for target a: (blob, mask, cell, disc — bool [D, D] each —, b, c, the clamped position)."""
    h, w = frame.shape
    mask, disc, seed, b, c, p = BLR.mask_at(frame, positions[a], R, fill, darker, min_contrast)
    cell = cell_at(p, a, positions, R, h, w)
    blob = BLR.flood(mask & cell, seed, connectivity)
    return blob, mask, cell, disc, b, c, p


def sums_at(frame, positions, a, R, fill, darker, min_contrast, connectivity):
    """Steps 1 - 6 for target a of the set `positions` on `frame`: (the twelve integers [12] int64, the clamped position)."""
    blob, mask, cell, disc, b, c, p = parts_at(frame, positions, a, R, fill, darker, min_contrast, connectivity)
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    y, x = dy[blob].astype(np.int64), dx[blob].astype(np.int64)
    rival = np.pad(mask & ~cell, 1)
    near = rival[:-2, 1:-1] | rival[2:, 1:-1] | rival[1:-1, :-2] | rival[1:-1, 2:]       # an edge neighbour on a rival's side
    return np.array([blob.sum(), y.sum(), x.sum(), (y * y).sum(), (y * x).sum(), (x * x).sum(), b, c, mask.sum(),
                     (blob & BLR.rim(disc)).sum(), (mask & cell).sum(), (blob & near).sum()], np.int64), p


def split_blobs(frames, ij, frame_index=None, radius=25, fill=128, darker=True, min_contrast=8, connectivity=8):
    """ij [n_sets, n_targets, 2] as pdog_blob_split writes it, set-major: (shape [n_sets, n_targets, 6] float64, sums [n_sets,
    n_targets, 12] int32).  frame_index None (set s on frame s) or [n_sets, n_targets]."""
    ij = np.asarray(ij)
    ns, nt = ij.shape[:2]
    out, words = np.empty((ns, nt, 6)), np.empty((ns, nt, 12), np.int32)
    for s in range(ns):
        for a in range(nt):
            f = frames[s if frame_index is None else int(frame_index[s][a])]
            v, p = sums_at(f, ij[s], a, radius, fill, darker, min_contrast, connectivity)
            words[s, a] = v
            out[s, a] = derive(v[:8], p)
    return out, words
