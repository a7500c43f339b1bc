"""What the background model must reproduce (include/pawsome_background.h), restated in NumPy, and the whole
track_video(background=...) flow over the Float64 oracle's functor, chunk-free: the model, the subtracted selected frames all
at once, the fill as the mode of the first of them, the bootstrap on it and one loop over the rest — plain, predicted, exclusive
or with the motion model, the last three through the restatements those rules already have.  TEST HELPER: nothing here loads
the library under test.

    model         np.sort(frames[samples], axis=0)[(K - 1) // 2]
    subtraction   clip(128 + int16(frame) - int16(model), 0, 255)
    samples       table[i * m // K'] for i in range(K'), K' = min(K, m)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusive_restatement as er  # noqa: E402
import motion_restatement as mr  # noqa: E402
import peaks_restatement as pr  # noqa: E402
import predict_restatement as qr  # noqa: E402

MAX_SAMPLES = 64     # PDOG_BG_MAX_SAMPLES


def samples(table, k):
    table = [int(v) for v in table]
    m = len(table)
    assert m >= 1 and 1 <= k <= MAX_SAMPLES
    n = min(k, m)
    return [table[i * m // n] for i in range(n)]


def median(frames, sample_list):
    """The lower median of frames[sample_list], uint8 [h, w]; a frame named twice counts twice."""
    s = [int(v) for v in sample_list]
    assert 1 <= len(s) <= MAX_SAMPLES
    return np.sort(np.asarray(frames)[s], axis=0)[(len(s) - 1) // 2]


def subtract(frames, model):
    """clamp(128 + frame - model, 0, 255) of one frame [h, w] or a stack [n, h, w], in int16."""
    d = 128 + np.asarray(frames).astype(np.int16) - np.asarray(model).astype(np.int16)
    return np.clip(d, 0, 255).astype(np.uint8)


def model_of(frames, table, background):
    """background: an int K -> the median of samples(table, K); an array -> that image."""
    return median(frames, samples(table, background)) if np.isscalar(background) else np.asarray(background, np.uint8)


def track_video(oracle, frames, table, background, tw, ws, darker, starts, loop="plain", min_distance=None, min_ratio=0.5,
                min_response=0.0, coast=8):
    """The flow: frames host uint8 [n, h, w], table the selected frames, starts one 1-based (row, col) guess per target (the
    functor is applied to it on the first subtracted frame, src/PawsomeTracker.jl:92-97), ws the side of the square window.
    Returns (positions int32 [n_targets, m, 2], state int32 [n_targets, m] or None, the subtracted frames, the fill)."""
    table = [int(v) for v in table]
    sub = subtract(np.asarray(frames)[table], model_of(frames, table, background))
    m, hw = len(table), sub.shape[1:]
    fill = oracle.mode_u8(sub[0])
    K = oracle.dog_kernel(oracle.sigma(tw), darker)
    radii = (ws // 2, ws // 2)
    nt = len(starts)
    out = np.zeros((nt, m, 2), np.int32)
    state = np.zeros((nt, m), np.int32)
    out[:, 0] = [oracle.detect(sub[0], fill, K, radii, g) for g in starts]
    if loop == "plain":
        for t in range(nt):
            for k in range(1, m):
                out[t, k] = oracle.detect(sub[k], fill, K, radii, out[t, k - 1])
        return out, None, sub, fill
    if loop == "predict":
        for t in range(nt):
            out[t], state[t], _ = qr.walk(oracle, sub, fill, K, radii, np.arange(m), out[t, 0], min_response, coast, first=1)
        return out, state, sub, fill
    # the joint loops: every target's window yields its k best separated peaks, the rule shares them out
    k = min(pr.MAX_K, 2 * nt)
    d = pr.default_min_distance(tw) if min_distance is None else int(min_distance)
    mstate = np.zeros((nt, 4), np.int32)
    for s in range(1, m):
        prev = out[:, s - 1]
        at = [qr.prediction(prev[t], mstate[t], hw) for t in range(nt)] if loop == "motion" else [tuple(int(v) for v in p) for p in prev]
        lists = []
        for t in range(nt):
            q, R = oracle.detect(sub[s], fill, K, radii, at[t], want_resp=True)
            lists.append(pr.select(R.astype(np.float32), at[t], radii, hw, q, k, d))
        ij, peak, count = np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]), np.array([l[2] for l in lists], np.int32)
        if loop == "motion":
            out[:, s], state[:, s], _, mstate = mr.step(prev, mstate, ij, peak, count, hw, d, min_ratio, min_response, coast)
        else:
            assert loop == "exclusive"
            out[:, s], state[:, s] = er.assign(prev, ij, peak, count, d, min_ratio)
    return out, state, sub, fill
