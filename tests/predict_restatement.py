"""NumPy restatement of the predicted chain (include/pawsome_predict.h) over the dense Float64 oracle, no GPU.

One step of one clip in an h x w frame.  The clip carries the position p filed last (the start, as given, before the first
step), the velocity v and n_held; min_response m >= 0 finite, coast >= 0:
    prediction   c = clamp(p + v) into rows 1 ... h, columns 1 ... w
    window       centred on c: R = float32(maximum of the window's response map), q = the functor's clamped position
    assigned     iff R > float32(m) (a NaN fails): p' = q, state 1, n_held' = 0, v' = p' - p (wrapping at 32 bits)
    held         otherwise: state -1, p' = c, n_held' = n_held + 1 (stays at 2^31 - 1), v' = v while n_held' < coast, else (0, 0)
    next guess   clamp(p' + v')
This is tests/motion_restatement.py at T = 1, k = 1 (tests/test_predict_cpu.py holds it to that).  `walk` is the walk of
pdog_detect_chains_predicted over a frame table, the window's map and position taken from the oracle.  Test code only: the
library never imports it."""
import numpy as np

INT32_MAX = 2**31 - 1


def clamp(x, n):
    return min(max(int(x), 1), int(n))


def _wrap32(x):
    return (int(x) + 2**31) % 2**32 - 2**31


def prediction(p, mstate, hw):
    return clamp(int(p[0]) + int(mstate[0]), hw[0]), clamp(int(p[1]) + int(mstate[1]), hw[1])


def step(p, mstate, R, q, hw, m, coast):
    """p (row, col); mstate (v_row, v_col, n_held, ...); R the float32 maximum of the window at prediction(p, mstate, hw); q the
    functor's position there.  Returns (p' (row, col), state, next guess (row, col), mstate' [4] int32)."""
    assert 0.0 <= m < np.inf and coast >= 0
    v, nh = [int(mstate[0]), int(mstate[1])], int(mstate[2])
    c = prediction(p, mstate, hw)
    with np.errstate(invalid="ignore"):
        hit = bool(np.float32(R) > np.float32(m))
    if hit:
        p2, state, nh = (int(q[0]), int(q[1])), 1, 0
        v = [_wrap32(p2[0] - int(p[0])), _wrap32(p2[1] - int(p[1]))]
    else:
        p2, state, nh = c, -1, min(nh + 1, INT32_MAX)
        if not nh < coast:
            v = [0, 0]
    new = np.array([v[0], v[1], nh, 0], np.int32)
    return p2, state, (clamp(p2[0] + v[0], hw[0]), clamp(p2[1] + v[1], hw[1])), new


def walk(oracle, frames, fill, Kn, radii, row, start, m, coast, first=0, mstate=None):
    """The walk of one clip over table row `row` (it ends where the row turns negative) from `start`.  Returns (out int32
    [n_steps, 2], state int32 [n_steps], mstate int32 [4]): steps at and beyond the clip's end stay 0, and a clip without a
    step returns the mstate it was given (zeros for None)."""
    hw = frames.shape[1:]
    row = np.asarray(row)
    n = len(row)
    length = int((row >= 0).sum())
    assert (row[:length] >= 0).all() and (row[length:] < 0).all()
    out, state = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    ms = np.zeros(4, np.int32) if mstate is None else np.asarray(mstate, np.int32).copy()
    p = (int(start[0]), int(start[1]))
    if first and length >= 1:
        out[0] = p
    for s in range(first, length):
        c = prediction(p, ms, hw)
        q, resp = oracle.detect(frames[int(row[s])], fill, Kn, radii, c, want_resp=True)
        p, state[s], _, ms = step(p, ms, np.float32(np.max(resp)), q, hw, m, coast)
        out[s] = p
    return out, state, ms
