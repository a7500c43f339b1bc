"""NumPy restatement of the frame-blob rule (include/pawsome_frame_blobs.h) over scipy.ndimage.label, and of the start rule of
track_video(find="frame"), no GPU.  The GPU's counts and words are tested bit for bit against this file
(tests/test_gpu_frame_blobs.py); tests/test_frame_blobs_cpu.py holds it to a plain pixel flood fill on every scene.

    mask      level - p >= min_contrast (darker) or p - level >= min_contrast
    blobs     the mask's connected components, connectivity 4 or 8
    words     n, Sy, Sx, Syy, Syx, Sxx, rmin, rmax, cmin, cmax, first, Ss per blob: int64, rows and columns 0-based
    kept      min_area <= n <= max_area, listed in ascending `first`; count = their number, the first `cap` are written
    derived   row, col (1-based), theta, major, minor, width in Float64 from exact integer numerators
Test code only: the library never imports it."""
import math

import numpy as np

WORDS = 12
N, SY, SX, SYY, SYX, SXX, RMIN, RMAX, CMIN, CMAX, FIRST, SS = range(WORDS)


def contrast(frame, level, darker):
    f = np.asarray(frame).astype(np.int64)
    return level - f if darker else f - level


def mask_of(frame, level, darker, min_contrast):
    return contrast(frame, level, darker) >= min_contrast


def words_of(labels, n_labels, s):
    """The twelve words of the components 1 ... n_labels of a label image (0: no component), [n_labels, 12] int64 in ascending
    `first`.  Every sum is formed in int64 (np.add.at): nothing here passes through a float."""
    h, w = labels.shape
    out = np.zeros((n_labels, WORDS), np.int64)
    if n_labels == 0:
        return out
    rr, cc = np.nonzero(labels)
    k = labels[rr, cc].astype(np.int64) - 1
    rr, cc = rr.astype(np.int64), cc.astype(np.int64)
    for col, v in ((N, np.ones_like(rr)), (SY, rr), (SX, cc), (SYY, rr * rr), (SYX, rr * cc), (SXX, cc * cc), (SS, s[rr, cc])):
        np.add.at(out[:, col], k, v)
    out[:, RMIN], out[:, CMIN], out[:, FIRST] = h, w, h * w
    out[:, RMAX] = out[:, CMAX] = -1
    np.minimum.at(out[:, RMIN], k, rr)
    np.maximum.at(out[:, RMAX], k, rr)
    np.minimum.at(out[:, CMIN], k, cc)
    np.maximum.at(out[:, CMAX], k, cc)
    np.minimum.at(out[:, FIRST], k, rr * w + cc)
    return out[np.argsort(out[:, FIRST], kind="stable")]


def all_blobs(frame, level=128, darker=True, min_contrast=8, connectivity=8):
    """Every blob of one frame, unfiltered: (words [n_blobs, 12] in ascending first, n_mask)."""
    from scipy import ndimage
    assert connectivity in (4, 8)
    s = contrast(frame, level, darker)
    mask = s >= min_contrast
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)       # the cross, or the full 3 x 3
    lab, n = ndimage.label(mask, structure=structure)
    return words_of(lab, n, s), int(mask.sum())


def find(frames, table=None, level=128, darker=True, min_contrast=8, connectivity=8, min_area=1, max_area=None, cap=64):
    """What FrameBlobs.find returns, on the host: (count int32 [n_steps, 2], words int64 [n_steps, cap, 12])."""
    frames = np.asarray(frames)
    table = range(len(frames)) if table is None else table
    if max_area is None:
        max_area = frames.shape[1] * frames.shape[2]
    count = np.zeros((len(table), 2), np.int32)
    words = np.zeros((len(table), cap, WORDS), np.int64)
    for k, f in enumerate(table):
        w, n_mask = all_blobs(frames[f], level, darker, min_contrast, connectivity)
        kept = w[(w[:, N] >= min_area) & (w[:, N] <= max_area)]
        count[k] = len(kept), n_mask
        words[k, :min(len(kept), cap)] = kept[:cap]
    return count, words


def derive(words):
    """[..., 12] integers -> [..., 6] float64: pawsome_shape.h's step 7 on the blob's sums, the centroid 1-based.  The
    numerators are Python integers (exact); the first floating-point operation is their conversion."""
    a = np.asarray(words).reshape(-1, WORDS)
    out = np.full((len(a), 6), np.nan)
    for i, wd in enumerate(a):
        n, sy, sx, syy, syx, sxx = (int(v) for v in wd[:6])
        if n <= 0:
            continue
        nd, nn = float(n), float(n * n)
        A, B, C = float(n * syy - sy * sy), float(n * sxx - sx * sx), float(n * syx - sy * sx)
        myy, mxx, myx = A / nn + 1.0 / 12.0, B / nn + 1.0 / 12.0, C / nn
        two, dif, tot = 2.0 * myx, mxx - myy, mxx + myy
        t = math.hypot(two, dif)
        lo = (tot - t) / 2.0
        out[i] = (1.0 + float(sy) / nd, 1.0 + float(sx) / nd, 0.5 * math.atan2(two, dif), 4.0 * math.sqrt((tot + t) / 2.0),
                  4.0 * math.sqrt(lo if lo > 0.0 else 0.0), 2.0 * math.sqrt(nd / math.pi))
    return out.reshape(np.asarray(words).shape[:-1] + (6,))


# ---- the start rule of track_video(find="frame") ----
def start_area_limits(target_width):
    W = int(math.ceil(float(target_width)))
    return max(1, W * W // 5), 3 * W * W


def start_guesses(frame, level, darker, target_width, k, min_contrast=8, connectivity=8):
    """The k guesses, 1-based (row, col), largest blob first, and the number of kept blobs (fewer than k: the call raises)."""
    lo, hi = start_area_limits(target_width)
    w, _ = all_blobs(frame, level, darker, min_contrast, connectivity)
    kept = w[(w[:, N] >= lo) & (w[:, N] <= hi)]
    order = sorted(range(len(kept)), key=lambda i: (-int(kept[i, N]), int(kept[i, FIRST])))[:k]
    rc = derive(kept[order])[:, :2] if order else np.zeros((0, 2))
    return [(int(np.rint(r)), int(np.rint(c))) for r, c in rc], len(kept)
