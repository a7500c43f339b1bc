"""NumPy restatement of the motion step (include/pawsome_motion.h, csrc/dog_motion.hpp), over GIVEN peak lists, no GPU.
The GPU's positions, states, next guesses and mstate are tested bit for bit against this file applied to the picks detect_peaks
returned in the same test (tests/test_gpu_motion.py); tests/test_motion_cpu.py holds the rule itself to hand-made lists and the
library's host function to this file.

One joint step for one group of T <= 32 targets in an h x w frame.  Per target: position p, velocity v, n_held; its list
ij[t][0 .. k-1], peak[t][0 .. k-1] (float32), count[t] is detect_peaks at the prediction.  min_distance d >= 1, ratio rho in
[0, 1], min_response m >= 0 finite, coast c >= 0:
    prediction   c_t = clamp(p_t + v_t) into rows 1 ... h, columns 1 ... w
    admissible   (q = 0 or q < count[t]) and peak[t][q] > float32(m) and peak[t][q] >= float32(rho) * peak[t][0], the product
                 one float32 multiplication; pick 1 is not exempt
    D(t, q)      squared integer distance from ij[t][q] to c_t; 0xFFFFFFFF when either |difference| >= 65536, and never more
    head         the entry of smallest D among those admissible and not blocked (squared distance to a position assigned in
                 this step below d * d), ties to the smaller q
    round        among the heads of the unassigned targets the smallest D wins, ties to the larger value (-0 and +0 tie, a NaN
                 ranks as -inf), then to the smaller t; the step ends when no unassigned target has a head
    assigned     p' = the pick, state = its number 1 ... k, n_held' = 0; contested (p' within d of ANOTHER target's prediction,
                 assigned or not): v' = v; otherwise v' = p' - p (wrapping at 32 bits)
    held         state -1, n_held' = n_held + 1 (stays at 2^31 - 1), p' = c_t, v' = v while n_held' < c, (0, 0) otherwise; a
                 held target blocks nobody
    next guess   clamp(p' + v')
Test code only: the library never imports it."""
import numpy as np

MAX_TARGETS = 32     # PDOG_MOTION_MAX_TARGETS
FAR = 0xFFFFFFFF


def clamp(x, n):
    return min(max(int(x), 1), int(n))


def admissible(q, count, peak, m, rho):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool((q == 0 or q < count) and peak[q] > np.float32(m) and peak[q] >= np.float32(rho) * np.float32(peak[0]))


def dist2(i, j, ci, cj):
    di, dj = int(i) - int(ci), int(j) - int(cj)
    if abs(di) >= 65536 or abs(dj) >= 65536:
        return FAR
    return min(di * di + dj * dj, FAR)


def _rank(v):
    v = float(v)
    return -np.inf if v != v else v


def _wrap32(x):
    return (int(x) + 2**31) % 2**32 - 2**31


def step(prev, mstate, ij, peak, count, hw, min_distance, rho, m, coast, detail=False):
    """One group: prev [T, 2], mstate [T, >= 3] (v_row, v_col, n_held), ij [T, k, 2], peak float32 [T, k], count [T].
    Returns (positions int32 [T, 2], state int32 [T], next guesses int32 [T, 2], mstate int32 [T, 4]) — and with detail a bool
    [T], which targets were contested."""
    prev, mstate, ij, count = np.asarray(prev, np.int64), np.asarray(mstate, np.int64), np.asarray(ij, np.int64), np.asarray(count)
    peak = np.asarray(peak, np.float32)
    T, k = peak.shape
    assert 1 <= T <= MAX_TARGETS and 1 <= k <= 32 and min_distance >= 1 and 0.0 <= rho <= 1.0 and 0.0 <= m < np.inf and coast >= 0
    h, w = hw
    d2 = int(min_distance) ** 2
    pred = [(clamp(prev[t, 0] + mstate[t, 0], h), clamp(prev[t, 1] + mstate[t, 1], w)) for t in range(T)]
    state = np.full(T, -1, np.int32)
    out = np.array(pred, np.int64).reshape(T, 2)
    taken = []
    for _ in range(T):
        best = None                              # (D, -rank, t, q): the smallest wins
        for t in range(T):
            if state[t] != -1:
                continue
            head = None
            for q in range(k):
                if not admissible(q, int(count[t]), peak[t], m, rho):
                    continue
                i, j = int(ij[t, q, 0]), int(ij[t, q, 1])
                if any((i - a) ** 2 + (j - b) ** 2 < d2 for a, b in taken):
                    continue
                D = dist2(i, j, *pred[t])
                if head is None or D < head[0]:  # (q ascending: an equal D does not replace)
                    head = (D, q)
            if head is None:
                continue
            cand = (head[0], -_rank(peak[t, head[1]]), t, head[1])
            if best is None or cand[:3] < best[:3]:
                best = cand
        if best is None:
            break
        _, _, t, q = best
        out[t] = ij[t, q]
        state[t] = q + 1
        taken.append((int(ij[t, q, 0]), int(ij[t, q, 1])))
    new = np.zeros((T, 4), np.int64)
    contested = np.zeros(T, bool)
    for t in range(T):
        v, nh = [int(mstate[t, 0]), int(mstate[t, 1])], int(mstate[t, 2])
        if state[t] == -1:
            nh = min(nh + 1, 2**31 - 1)
            if not nh < coast:
                v = [0, 0]
        else:
            a, b = int(out[t, 0]), int(out[t, 1])
            contested[t] = any(u != t and (a - pred[u][0]) ** 2 + (b - pred[u][1]) ** 2 < d2 for u in range(T))
            if not contested[t]:
                v = [_wrap32(a - int(prev[t, 0])), _wrap32(b - int(prev[t, 1]))]
            nh = 0
        new[t] = (v[0], v[1], nh, 0)
    nxt = np.array([(clamp(out[t, 0] + new[t, 0], h), clamp(out[t, 1] + new[t, 1], w)) for t in range(T)], np.int64).reshape(T, 2)
    res = (out.astype(np.int32), state, nxt.astype(np.int32), new.astype(np.int32))
    return res + (contested,) if detail else res


def step_groups(prev, mstate, ij, peak, count, hw, min_distance, rho, m, coast):
    """The same for G groups: prev [G, T, 2], mstate [G, T, 4], ij [G, T, k, 2], peak [G, T, k], count [G, T]."""
    res = [step(prev[g], mstate[g], ij[g], peak[g], count[g], hw, min_distance, rho, m, coast) for g in range(len(prev))]
    return tuple(np.stack([r[i] for r in res]) for i in range(4))
