"""NumPy restatement of the K-peaks rule (include/pawsome_peaks.h, csrc/dog_peaks.hpp), over a GIVEN response map, no GPU.
The GPU's picks are tested bit for bit against this file applied to the map the same call returned
(tests/test_gpu_peaks.py); tests/test_peaks_cpu.py holds the rule itself to hand-made maps.

For one window with guess g, radii r and an H x W frame, R is the window's response as an h x w array (win_h rows, win_w
columns; the library's column-major map is R.T flattened: idx = col * win_h + row), window pixel (row, col) being frame pixel
(g1 - r1 + row, g2 - r2 + col), 1-based:
    pick 1       the position the detect call returned (given here as `pick1`, already clamped, src/PawsomeTracker.jl:61);
                 its value is the maximum of R over the whole window, NaNs left out (the first idx that holds it; -inf for
                 a window of NaNs)
    candidates   window pixels that (a) lie inside the frame, (b) are a local maximum among their up to eight neighbours IN
                 THE WINDOW — R(p) > R(q) for a neighbour of smaller idx, R(p) >= R(q) for one of larger idx —, (c) hold no NaN
    pick k >= 2  the candidate of largest R, ties to the smallest idx, whose squared distance di*di + dj*dj (integers) to every
                 earlier pick is at least min_distance**2; the selection ends when no candidate is left
    outputs      count in 1 ... K, 1-based (row, col), float32 values; beyond count (0, 0) and -inf
min_distance None or <= 0: ceil(target_width), at least 1.
Test code only: the library never imports it."""
import math

import numpy as np

MAX_K = 32          # PDOG_PEAKS_MAX_K
LIST_CAPACITY = 1536  # PEAKS_LIST (csrc/dog_peaks.hpp): candidates the kernel's LDS list holds


def default_min_distance(target_width):
    return max(1, int(math.ceil(float(target_width))))


def local_maxima(R):
    """(b) and (c): a bool mask over the h x w map R."""
    R = np.asarray(R)
    n1, n2 = R.shape
    ok = ~np.isnan(R)
    with np.errstate(invalid="ignore"):
        for dc in (-1, 0, 1):
            for dr in (-1, 0, 1):
                if dr == 0 and dc == 0:
                    continue
                a0, a1 = max(0, -dr), min(n1, n1 - dr)        # the pixels whose neighbour (row + dr, col + dc) lies in the window
                b0, b1 = max(0, -dc), min(n2, n2 - dc)
                if a1 <= a0 or b1 <= b0:
                    continue
                p, q = R[a0:a1, b0:b1], R[a0 + dr:a1 + dr, b0 + dc:b1 + dc]
                smaller = dc < 0 or (dc == 0 and dr < 0)      # the neighbour's idx = (col + dc) * n1 + row + dr is the smaller one
                ok[a0:a1, b0:b1] &= (p > q) if smaller else (p >= q)
    return ok


def candidates(R, guess, radii, frame_hw):
    """[(value, idx, frame row, frame col)] of every candidate, sorted by value descending, idx ascending."""
    R = np.asarray(R)
    n1, n2 = R.shape
    f1, f2 = int(guess[0]) - int(radii[0]), int(guess[1]) - int(radii[1])
    rows, cols = np.nonzero(local_maxima(R))
    fi, fj = rows + f1, cols + f2
    keep = (fi >= 1) & (fi <= frame_hw[0]) & (fj >= 1) & (fj <= frame_hw[1])
    rows, cols, fi, fj = rows[keep], cols[keep], fi[keep], fj[keep]
    vals = R[rows, cols]
    idx = cols.astype(np.int64) * n1 + rows
    order = np.lexsort((idx, -vals.astype(np.float64)))       # (-0.0 and 0.0 compare equal: the idx decides)
    return [(vals[o], int(idx[o]), int(fi[o]), int(fj[o])) for o in order]


def window_max(R):
    """Pick 1's value: the maximum over the window without its NaNs, the value at the first idx that holds it."""
    flat = np.asarray(R).T.ravel()                             # idx order
    if np.isnan(flat).all():
        return np.float32(-np.inf)
    return np.float32(flat[np.nanargmax(flat)])


def select(R, guess, radii, frame_hw, pick1, k, min_distance):
    """(ij int32 [k, 2], peak float32 [k], count) of one window; min_distance a positive integer."""
    assert 1 <= k <= MAX_K and min_distance >= 1
    md2 = int(min_distance) ** 2
    ij = np.zeros((k, 2), np.int32)
    peak = np.full(k, -np.inf, np.float32)
    picks = [(int(pick1[0]), int(pick1[1]))]
    ij[0], peak[0] = picks[0], window_max(R)
    if k > 1:
        for v, _, fi, fj in candidates(R, guess, radii, frame_hw):
            if all((fi - pi) ** 2 + (fj - pj) ** 2 >= md2 for pi, pj in picks):
                ij[len(picks)], peak[len(picks)] = (fi, fj), np.float32(v)
                picks.append((fi, fj))
                if len(picks) == k:
                    break
    return ij, peak, len(picks)


def select_batch(resp, guesses, radii, frame_hw, pick1, k, min_distance):
    """The same for n windows; resp [n, win_w, win_h] as BatchTracker.detect hands it out (resp[b].T is the h x w map)."""
    out = [select(np.asarray(resp[b]).T, guesses[b], radii, frame_hw, pick1[b], k, min_distance) for b in range(len(resp))]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32))


def n_candidates(R, guess, radii, frame_hw):
    return len(candidates(R, guess, radii, frame_hw))
