"""NumPy restatement of the pre-pass's SECOND stage (csrc/dog_prune.hpp, "the cell bound"): inside every slot's first-stage hull
(tests/prune_restatement.py, imported unchanged) a bound per 8 × 8 output cell,
    B(yb, xb) = Σ_{dy, dx < NS} Wq[dy][dx] · r[yb + dy][xb + dx],
in the device's exact integer arithmetic: r = ⌈16·√Ec⌉ of every 8 × 8 input cell's energy about the window's DC level (0 outside
the tile), Wq = ⌈2¹²·W/‖K‖₂⌉ as the host forms them (csrc/pdog_math.cpp, dog_refine_weights, restated here operation for
operation) and the threshold ⌊2¹⁶·q·(1 − 2⁻³⁰)⌋, q = (L − 2δ(V) − T_max)·255/‖K‖₂ the first stage's own.  A block of a slot stays
iff the first stage keeps it and one of the output cells that meet the slot's columns has B ≥ the threshold; the refined
range is the hull of those.  Test code only: the library never imports it."""
import math

import numpy as np

import fp32_restatement as fr
import prune_restatement as pr

CH = pr.CH
W_BITS, R_SCALE = 12, 16
MAX_SPAN = 32                       # csrc/dog_prune.hpp, PRUNE_REFINE_MAX_SPAN: a row of NS terms stays below 2³²


def box_tables(gp, gm, f32):
    """Σ g₊², Σ g₋², Σ g₊g₋ over the kernel rows [8d − i, 8d − i + 8) ∩ [0, l) for d < NS, i < 8, from sequential prefix sums."""
    l = len(gp)
    NS = pr.span(l)
    a = [float(np.float32(v)) if f32 else float(v) for v in gp]
    b = [float(np.float32(v)) if f32 else float(v) for v in gm]
    pp, mm, pm = [0.0], [0.0], [0.0]
    for k in range(l):
        pp.append(pp[-1] + a[k] * a[k])
        mm.append(mm[-1] + b[k] * b[k])
        pm.append(pm[-1] + a[k] * b[k])
    A, Bm, Cm = np.zeros((NS, 8)), np.zeros((NS, 8)), np.zeros((NS, 8))
    for d in range(NS):
        for i in range(8):
            lo, hi = min(max(8 * d - i, 0), l), min(max(8 * d - i + 8, 0), l)
            A[d, i], Bm[d, i], Cm[d, i] = pp[hi] - pp[lo], mm[hi] - mm[lo], pm[hi] - pm[lo]
    return A, Bm, Cm


def box_norm2(tabs, dy, i, dx, j):
    A, Bm, Cm = tabs
    ab = float(A[dy, i]) * float(A[dx, j])
    ab = ab + float(Bm[dy, i]) * float(Bm[dx, j])
    cc = float(Cm[dy, i]) * float(Cm[dx, j])
    return ab - 2.0 * cc


def weights(gp, gm):
    """Wq [NS][NS] (Python ints): the largest partial norm over the 64 offsets and both tap roundings, a slack of 1e-14·‖K‖₂² for
    the cancellation in the box sums, rounded up in units of ‖K‖₂ / 2¹²."""
    NS = pr.span(len(gp))
    norm = pr.kernel_norm_up(gp, gm)
    tabs = (box_tables(gp, gm, True), box_tables(gp, gm, False))
    out = [[0] * NS for _ in range(NS)]
    for dy in range(NS):
        for dx in range(NS):
            w2 = 0.0
            for t in tabs:
                for i in range(8):
                    for j in range(8):
                        w2 = max(w2, box_norm2(t, dy, i, dx, j))
            w2 = w2 + 1e-14 * (norm * norm)
            out[dy][dx] = int(math.ceil(4096.0 * (math.sqrt(w2) / norm)))
    return out


_WEIGHTS = {}


def weights_of(tw, darker=True):
    if tw not in _WEIGHTS:
        gp, gm, _, _ = fr.tap_tables(tw, darker)
        _WEIGHTS[tw] = np.array(weights(gp, gm), dtype=object)
    return _WEIGHTS[tw]


def cell_roots(tile, dc):
    """r [nsub + 1][ncx + 1]: ⌈16·√Ec⌉ per 8 × 8 cell of the tile, a zero row and column behind them."""
    NA, TWin = tile.shape
    nsub, ncx = -(-NA // CH), -(-TWin // 8)
    vp = np.zeros((nsub * CH, ncx * 8), np.int64)
    vp[:NA, :TWin] = tile.astype(np.int64) - dc
    Ec = (vp * vp).reshape(nsub, CH, ncx, 8).sum((1, 3))
    r = np.zeros((nsub + 1, ncx + 1), dtype=object)
    for y in range(nsub):
        for x in range(ncx):
            e = int(Ec[y, x])
            r[y, x] = 0 if e == 0 else math.isqrt(R_SCALE * R_SCALE * e - 1) + 1
    return r


def refine(tile, fill, tw, darker, pp=None):
    """pp: prune_restatement.prepass of the same arguments.  Returns a dict: the refined range per slot (`hull`), the integer
    threshold `tq` (None: the second stage does not run) and B per (block, output cell) where it was evaluated (`B`)."""
    pp = pp or pr.prepass(tile, fill, tw, darker)
    gp, gm, _, _ = fr.tap_tables(tw, darker)
    l = len(gp)
    NS = pp["span"]
    out = dict(hull=list(pp["hull"]), tq=None, B={})
    if pp["emax"] < 0.0 or NS > MAX_SPAN:
        return out
    thr = pp["L"] - 2.0 * pp["dV"] - pp["Tmax"]
    q = thr * (255.0 / pp["norm"])
    tq = int(math.floor(q * 65536.0 * (1.0 - 2.0 ** -30)))
    Wq = weights_of(tw, darker)
    r = cell_roots(tile, pp["dc"])
    nsub1, ncx1 = r.shape
    hull = []
    for (c0, w), (ba, bb) in zip(pp["slots"], pp["hull"]):
        keep = []
        for j in range(ba, bb):
            for xb in range(c0 >> 3, ((c0 + w - 1) >> 3) + 1):
                B = 0
                for dy in range(min(NS, nsub1 - j)):
                    for dx in range(min(NS, ncx1 - xb)):
                        B += int(Wq[dy][dx]) * int(r[j + dy, xb + dx])
                out["B"][(j, xb)] = B
                if B >= tq:
                    keep.append(j)
        hull.append((keep[0], keep[-1] + 1) if keep else (0, 0))
    out.update(hull=hull, tq=tq, thr=thr)
    return out


def kept_pairs(hull, l, nsub):
    return sum((min(nsub, bb + pr.tail(l)) - ba) if bb > ba else 0 for ba, bb in hull)
