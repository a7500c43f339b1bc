"""NumPy restatement of the exclusive step (include/pawsome_exclusive.h, csrc/dog_assign.hpp), over GIVEN peak lists, no GPU.
The GPU's positions and states are tested bit for bit against this file applied to the picks detect_peaks returned in the
same test (tests/test_gpu_exclusive.py); tests/test_exclusive_cpu.py holds the rule itself to hand-made lists and the
library's host function to this file.

One joint step for one group of T <= 32 targets with previous positions prev[t] and, per target, a list ij[t][0 .. k-1],
peak[t][0 .. k-1] (float32), count[t]; min_distance d >= 1, ratio rho in [0, 1]:
    admissible   entry 0 always; entry q >= 1 when q < count[t], peak[t][q] > 0 and peak[t][q] >= float32(rho) * peak[t][0],
                 the product one float32 multiplication
    head         the first entry of a target's list, in list order, that is admissible and not blocked; blocked: squared
                 integer distance to a position already assigned in this step below d * d
    round        among the heads of the targets not yet assigned the largest value wins (-0 and +0 tie, a NaN ranks as -inf),
                 ties to the smaller t; the winner is assigned that position; the step ends when no unassigned target has a head
    outputs      assigned: the position, state = the pick's number 1 ... k; never assigned (held): prev[t], state -1; a held
                 target blocks nobody
Test code only: the library never imports it."""
import numpy as np

MAX_TARGETS = 32     # PDOG_EXCLUSIVE_MAX_TARGETS


def admissible(q, count, peak, rho):
    if q == 0:
        return True
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(q < count and peak[q] > 0 and peak[q] >= np.float32(rho) * np.float32(peak[0]))


def _rank(v):
    """The value as the round compares it: a NaN as -inf; Python compares -0.0 and 0.0 equal."""
    v = float(v)
    return -np.inf if v != v else v


def assign(prev, ij, peak, count, min_distance, rho):
    """(positions int32 [T, 2], state int32 [T]) of one group: prev [T, 2], ij [T, k, 2], peak float32 [T, k], count [T]."""
    prev, ij, count = np.asarray(prev, np.int64), np.asarray(ij, np.int64), np.asarray(count)
    peak = np.asarray(peak, np.float32)
    T, k = peak.shape
    assert 1 <= T <= MAX_TARGETS and 1 <= k <= 32 and min_distance >= 1 and 0.0 <= rho <= 1.0
    d2 = int(min_distance) ** 2
    out = prev.copy()
    state = np.full(T, -1, np.int32)
    taken = []                                   # positions assigned so far, Python integers
    for _ in range(T):
        best = None                              # (rank, -t, q)
        for t in range(T):
            if state[t] != -1:
                continue
            for q in range(k):
                if not admissible(q, int(count[t]), peak[t], rho):
                    continue
                i, j = int(ij[t, q, 0]), int(ij[t, q, 1])
                if any((i - a) ** 2 + (j - b) ** 2 < d2 for a, b in taken):
                    continue
                if best is None or _rank(peak[t, q]) > best[0]:      # (t ascending: an equal value does not replace)
                    best = (_rank(peak[t, q]), t, q)
                break                            # the head is the FIRST such entry
        if best is None:
            break
        _, t, q = best
        out[t] = ij[t, q]
        state[t] = q + 1
        taken.append((int(ij[t, q, 0]), int(ij[t, q, 1])))
    return out.astype(np.int32), state


def assign_groups(prev, ij, peak, count, min_distance, rho):
    """The same for G groups: prev [G, T, 2], ij [G, T, k, 2], peak [G, T, k], count [G, T]."""
    res = [assign(prev[g], ij[g], peak[g], count[g], min_distance, rho) for g in range(len(prev))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
