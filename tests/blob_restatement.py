"""NumPy restatement of the blob rule (include/pawsome_blob.h): steps 1 - 5 as tests/shape_restatement.py has them, the seed,
a pixel flood fill with an explicit stack for the blob, the ten integers in int64, and shape_restatement.derive on the first
eight.  Written from the header's text, not from the library's code.  TEST HELPER: nothing here loads the library under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shape_restatement import _padded, derive  # noqa: E402

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def mask_at(frame, ij, R, fill, darker, min_contrast):
    """Steps 1 - 5a for one 1-based position: (mask bool [D, D] over the bounding box, disc bool [D, D], seed (row, col) in the
    box, b, c, the clamped position).  The mask is all False below min_contrast."""
    h, w = frame.shape
    i, j = min(max(int(ij[0]), 1), h), min(max(int(ij[1]), 1), w)
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    disc = dy * dy + dx * dx <= R * R
    p = _padded(frame, fill, i - 1 + dy, j - 1 + dx)
    vals = p[disc]
    b = int(np.sort(vals)[(len(vals) - 1) // 2])
    s = (b - p) if darker else (p - b)
    s3 = s[R - 1:R + 2, R - 1:R + 2]
    c = max(0, int(s3.max()))
    seed = None
    for y in range(3):                      # row-major: dy ascending, then dx
        for x in range(3):
            if seed is None and int(s3[y, x]) == c:
                seed = (R - 1 + y, R - 1 + x)
    mask = disc & (2 * s >= c) if c >= min_contrast else np.zeros_like(disc)
    return mask, disc, seed, b, c, (i, j)


def flood(mask, seed, connectivity):
    """The connected component of `mask` that contains `seed`: a plain pixel flood fill, explicit stack (on a flat copy of the
    mask with a border of zeros, so that no neighbour needs a bounds check)."""
    out = np.zeros_like(mask)
    if seed is None or not mask[seed]:
        return out
    D0, D1 = mask.shape
    w = D1 + 2
    todo = bytearray(np.pad(mask, 1).astype(np.uint8).tobytes())       # 1: a mask pixel not reached yet
    steps = [ey * w + ex for ey, ex in NEIGHBOURS[connectivity]]
    start = (seed[0] + 1) * w + seed[1] + 1
    todo[start] = 0
    stack, reached = [start], [start]
    while stack:
        at = stack.pop()
        for d in steps:
            if todo[at + d]:
                todo[at + d] = 0
                stack.append(at + d)
                reached.append(at + d)
    at = np.array(reached)
    out[at // w - 1, at % w - 1] = True
    return out


def rim(disc):
    """The disc pixels with at least one of their four edge neighbours outside the disc."""
    pad = np.pad(disc, 1)
    inner = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    return disc & ~inner


def sums_at(frame, ij, R, fill, darker, min_contrast, connectivity):
    """Steps 1 - 6 for one position: (the ten integers [10] int64, the clamped position)."""
    mask, disc, seed, b, c, q = mask_at(frame, ij, R, fill, darker, min_contrast)
    blob = flood(mask, seed, connectivity)
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    y, x = dy[blob].astype(np.int64), dx[blob].astype(np.int64)
    return np.array([blob.sum(), y.sum(), x.sum(), (y * y).sum(), (y * x).sum(), (x * x).sum(), b, c, mask.sum(),
                     (blob & rim(disc)).sum()], np.int64), q


def blobs(frames, ij, frame_index=None, radius=25, fill=128, darker=True, min_contrast=8, connectivity=8):
    """n positions as pdog_blob writes them: (shape [n, 6] float64, sums [n, 10] int32)."""
    ij = np.asarray(ij).reshape(-1, 2)
    out, words = np.empty((len(ij), 6)), np.empty((len(ij), 10), np.int32)
    for k, p in enumerate(ij):
        s, q = sums_at(frames[k if frame_index is None else int(frame_index[k])], p, radius, fill, darker, min_contrast, connectivity)
        words[k] = s
        out[k] = derive(s[:8], q)
    return out, words
