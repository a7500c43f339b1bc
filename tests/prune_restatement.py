"""NumPy restatement of the roll batch path's pre-pass (csrc/dog_prune.hpp): the Cauchy–Schwarz bound per 8-row output block
of every slot (64-column strip or remainder column), the lower bound L on the window's maximum, and the contiguous hull of
the blocks that cannot be excluded.  L is evaluated as the kernel evaluates it — from the 8 × 8 pixels' own input patch, in the
roll order (tests/fp32_restatement.py) — and NOT read off a response map, so tests/test_prune_cpu.py can hold it, the bound
and the hull against the map the kernels compute, and tests/test_gpu_prune.py the kernel's kept counts against this file's.
Test code only: the library never imports it."""
import math

import numpy as np

import fp32_restatement as fr

CH, TW, PB, THIN_MAX = 8, 64, 8, 6


def kernel_norm_up(gp, gm):
    """pdog_math.cpp, dog_kernel_norm_up: ‖g₊⊗g₊ − g₋⊗g₋‖₂ from the f32-rounded and the Float64 taps, the larger, rounded up."""
    def norm(a, b):
        pp, mm, pm = float(np.dot(a, a)), float(np.dot(b, b)), float(np.dot(a, b))
        return math.sqrt(max(0.0, pp * pp + mm * mm - 2.0 * pm * pm))
    n = max(norm(gp.astype(np.float32).astype(np.float64), gm.astype(np.float32).astype(np.float64)), norm(gp, gm))
    return float(np.nextafter(np.float32(n), np.float32(2.0)))


def slots(n2):
    """(first window column, window columns) of every slot: the strips, then the remainder columns (pawsome_dog.hip)."""
    r = n2 % TW
    thin = r if (n2 > TW and 0 < r <= THIN_MAX) else 0
    ncols = n2 - thin
    ns = -(-ncols // TW)
    out = [((min(s * TW, ncols - TW) if ncols >= TW else 0), min(TW, ncols)) for s in range(ns)]
    return out + [(ncols + k, 1) for k in range(thin)]


def span(l):
    return (CH + l - 1 + CH - 1) // CH


def tail(l):
    return (l - 1 + CH - 1) // CH


def thresholds(tw, darker):
    """(T, T_max) at V = 255 as exact_ctl forms them for the roll family."""
    gp, gm, _, _ = fr.tap_tables(tw, darker)
    l = len(gp)
    F = fr.factor(fr.order("roll", l), gp, gm)
    F_rescan = fr.factor(dict(row=[[(k, (k,)) for k in range(l)]], col=[list(range(l))], flush=False, col_mode="interleaved"), gp, gm)
    T = np.nextafter(np.float32(2.0 * fr.U * F * 1.02 + 2e-9), np.float32(1.0))
    T_rescan = np.nextafter(np.float32(fr.U * (F + F_rescan) * 1.02 + 2e-9), np.float32(1.0))
    return float(T), float(max(T, T_rescan))


def prepass(tile, fill, tw, darker, cell_darker=None):
    """tile: the window's padded tile.  Returns a dict: dc, V, E [slot][sub-chunk], the L block's origin, L, the exclusion
    threshold on ΣE (−1: nothing excluded) and the hull per slot.  cell_darker: the sign PruneGeo::darker gives the 3 × 3-cell
    sums, by default the target's own; a test passes the other one to state what a kernel with that sign wrong would keep."""
    gp, gm, _, _ = fr.tap_tables(tw, darker)
    l, hw = len(gp), len(gp) // 2
    NA, TWin = tile.shape
    n1, n2 = NA - l + 1, TWin - l + 1
    nsub, ncx = -(-NA // CH), -(-TWin // 8)
    dc = fr.dc_level(tile, fill)
    v = tile.astype(np.int64) - dc
    V = int(np.abs(v).max())
    vp = np.zeros((nsub * CH, ncx * 8), np.int64)
    vp[:NA, :TWin] = v
    band_col = (vp * vp).reshape(nsub, CH, -1).sum(1)                 # [sub-chunk][tile column]
    sl = slots(n2)
    E = np.array([[int(band_col[sc, c0:c0 + w + l - 1].sum()) for sc in range(nsub)] for c0, w in sl], np.int64)
    cell = vp.reshape(nsub, CH, ncx, 8).sum((1, 3))
    pad = np.zeros((nsub + 2, ncx + 2), np.int64)
    pad[1:-1, 1:-1] = cell
    s33 = sum(pad[1 + dy:1 + dy + nsub, 1 + dx:1 + dx + ncx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    if darker if cell_darker is None else cell_darker:
        s33 = -s33
    cy, cx = divmod(int(np.argmax(s33)), ncx)                         # the first maximum in row-major cell order
    ny, nx = min(PB, n1), min(PB, n2)
    oy = min(max(CH * cy + 4 - hw - PB // 2, 0), n1 - ny)
    ox = min(max(8 * cx + 4 - hw - PB // 2, 0), n2 - nx)
    # the 8 × 8 pixels from their own patch of the tile, window DC level, roll order: what dog_prune_kernel's row and column pass do
    patch = tile[oy:oy + ny + l - 1, ox:ox + nx + l - 1]
    L = float(fr.response_of_order(patch, fill, tw, darker, fr.order("roll", l), dc=dc).max())
    T, Tmax = thresholds(tw, darker)
    dV = 0.5 * T * (V * (1.0 / 255.0)) * 1.00001                     # (the kernel's own expression, operation for operation)
    thr = L - 2.0 * dV - Tmax
    q = thr * (255.0 / kernel_norm_up(gp, gm))
    emax = q * q * (1.0 - 2.0 ** -30) if thr > 0.0 else -1.0
    nblk, NS = -(-n1 // CH), span(l)
    hull = []
    for s in range(len(sl)):
        keep = [j for j in range(nblk) if float(E[s, j:j + NS].sum()) >= emax]
        hull.append((keep[0], keep[-1] + 1) if keep else (0, 0))
    return dict(dc=dc, V=V, E=E, origin=(oy, ox), L=L, emax=emax, hull=hull, slots=sl, T=T, Tmax=Tmax, dV=dV,
                norm=kernel_norm_up(gp, gm), span=NS, nsub=nsub, nblk=nblk)


def kept_pairs(pp, l):
    """(kept, total) (slot, sub-chunk) pairs as the pre-pass counts them."""
    kept = sum((min(pp["nsub"], bb + tail(l)) - ba) if bb > ba else 0 for ba, bb in pp["hull"])
    return kept, len(pp["hull"]) * pp["nsub"]
