"""NumPy restatement of the shape rule (include/pawsome_shape.h): steps 1 - 6 in int64, step 7 in float64, step 8 as a loop.
Written from the header's text, not from the library's code.  TEST HELPER: nothing here loads the library under test."""
import math

import numpy as np

MAX_RADIUS = 127
NAMES = ("row", "col", "theta", "major", "minor", "width")


def default_radius(target_width):
    return int(min(max(math.ceil(target_width), 2), MAX_RADIUS))


def disc_offsets(R):
    """(dy, dx) of the patch, each [N] int64, row-major."""
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    m = dy * dy + dx * dx <= R * R
    return dy[m].astype(np.int64), dx[m].astype(np.int64)


def _padded(frame, fill, rows, cols):
    """frame at 0-based (rows, cols), the fill outside (the PaddedView rule)."""
    h, w = frame.shape
    inside = (rows >= 0) & (rows < h) & (cols >= 0) & (cols < w)
    v = frame[np.clip(rows, 0, h - 1), np.clip(cols, 0, w - 1)].astype(np.int64)
    return np.where(inside, v, np.int64(fill))


def sums_at(frame, ij, R, fill, darker, min_contrast):
    """Steps 1 - 6 for one 1-based position on one frame: (the eight integers [8] int64, the clamped position)."""
    h, w = frame.shape
    i, j = min(max(int(ij[0]), 1), h), min(max(int(ij[1]), 1), w)
    dy, dx = disc_offsets(R)
    p = _padded(frame, fill, i - 1 + dy, j - 1 + dx)
    b = int(np.sort(p)[(len(p) - 1) // 2])
    s = (b - p) if darker else (p - b)
    y3, x3 = np.mgrid[-1:2, -1:2]
    p3 = _padded(frame, fill, i - 1 + y3, j - 1 + x3)
    c = max(0, int(((b - p3) if darker else (p3 - b)).max()))
    if c < min_contrast:
        return np.array([0, 0, 0, 0, 0, 0, b, c], np.int64), (i, j)
    m = 2 * s >= c
    y, x = dy[m], dx[m]
    return np.array([m.sum(), y.sum(), x.sum(), (y * y).sum(), (y * x).sum(), (x * x).sum(), b, c], np.int64), (i, j)


def derive(sums, ij):
    """Step 7: six float64 from the eight integers and the clamped position."""
    n, Sy, Sx, Syy, Syx, Sxx = (int(v) for v in sums[:6])
    if n == 0:
        return np.full(6, np.nan)
    f = np.float64
    A, B, C = n * Syy - Sy * Sy, n * Sxx - Sx * Sx, n * Syx - Sy * Sx         # exact (Python integers)
    nn = f(n * n)
    myy, mxx, myx = f(A) / nn + f(1.0) / f(12.0), f(B) / nn + f(1.0) / f(12.0), f(C) / nn
    two, dif, tot = f(2.0) * myx, mxx - myy, mxx + myy
    t = np.hypot(two, dif)
    lo = (tot - t) / f(2.0)
    return np.array([f(ij[0]) + f(Sy) / f(n), f(ij[1]) + f(Sx) / f(n), f(0.5) * np.arctan2(two, dif),
                     f(4.0) * np.sqrt((tot + t) / f(2.0)), f(4.0) * np.sqrt(max(lo, f(0.0))), f(2.0) * np.sqrt(f(n) / f(math.pi))], np.float64)


def shapes(frames, ij, frame_index=None, radius=25, fill=128, darker=True, min_contrast=8):
    """n positions as pdog_shape writes them: (shape [n, 6] float64, sums [n, 8] int32)."""
    ij = np.asarray(ij).reshape(-1, 2)
    out, words = np.empty((len(ij), 6)), np.empty((len(ij), 8), np.int32)
    for k, p in enumerate(ij):
        s, q = sums_at(frames[k if frame_index is None else int(frame_index[k])], p, radius, fill, darker, min_contrast)
        words[k] = s
        out[k] = derive(s, q)
    return out, words


def headings(theta, ij, min_step=1.0):
    """Step 8 for one target: theta [m], ij [m, 2] -> [m] float64."""
    f = np.float64
    pi = f(math.pi)
    out = np.empty(len(theta), np.float64)
    prev = None
    for k, th in enumerate(np.asarray(theta, np.float64)):
        if np.isnan(th):
            out[k] = np.nan
            continue
        flip = False
        d = None if k == 0 else (int(ij[k][0]) - int(ij[k - 1][0]), int(ij[k][1]) - int(ij[k - 1][1]))
        if d is not None and f(d[0]) * f(d[0]) + f(d[1]) * f(d[1]) >= f(min_step) * f(min_step):
            flip = f(d[0]) * np.sin(th) + f(d[1]) * np.cos(th) < 0
        elif prev is not None:
            e = th - prev
            if e > pi:
                e -= f(2.0) * pi
            elif e <= -pi:
                e += f(2.0) * pi
            flip = abs(e) > pi / f(2.0)
        hd = th + pi if flip else th
        if hd > pi:
            hd -= f(2.0) * pi
        out[k] = prev = hd
    return out
