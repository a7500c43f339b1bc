"""NumPy float32 restatement of the ORDER in which each kernel family adds its FP32 terms — the executable statement of
the premise exact mode rests on (csrc/dog_exact.hpp: "an a-priori bound that follows the kernel's own operation order").
The GPU's response maps are tested bit for bit against this file (tests/test_gpu_fp32_order.py), and the error-bound
factor of each family is derived from the same description the emulation runs (tests/test_fp32_order_cpu.py).

An ORDER is data, `order(family, l, ...)`:
    row       list of chains; a chain is a list of terms (k, offsets): one FMA  acc <- fl(acc + (sum of in[x + o], o in offsets) * g[k])
    col       list of chains; a chain is a list of taps t:              one FMA  acc <- fl(acc + R[y + t] * c[t])
    flush     False: each pass is ONE chain started from zero.  True: every chain starts from zero and its sum is added to a
              running total that starts from zero (dog_twopass.hpp, blocked accumulation): total <- fl(total + chain)
    col_mode  "interleaved": one f32 per output takes, per tap, the g+ term and then the g- term (roll kernels, thin and folded
              remainder columns);  "separate": a chain (or chains) per Gaussian, the two results added at the end
Both Gaussians of a pass see the same chains.  Every step is one rounding: an FMA is float32(float64(a) * float64(b) +
float64(c)) — the product of two float32 is exact in float64, and the one case in which rounding the float64 sum again
would differ from rounding once (the float64 sum lands exactly between two float32 values while the exact sum does not)
is settled with the sum's exact error term.  The pair sums of the symmetric row passes are exact (integers below 2^10).
Test code only: the library never imports it."""
import math

import numpy as np

U = 2.0 ** -24                 # unit roundoff of float32
TWOPASS_FLUSH_L = 101          # dog_twopass.hpp: blocked accumulation from this kernel length on
FAMILIES = ("roll", "ring", "fused", "tiled", "twopass")


# ---- the host's tables (pdog_math.cpp, pawsome_dog.hip: "taps: Float64 on the host, one rounding to f32") ----
def sigma_of(tw):
    return float(tw) / (2.0 * math.sqrt(2.0 * math.log(2.0)))


def kernel_len(sigma):
    return 4 * int(math.ceil(sigma * math.sqrt(2.0))) + 1


def gaussian_1d(sigma, l):
    w = l >> 1
    g = [math.exp(-(float(x) * float(x)) / (2.0 * sigma * sigma)) for x in range(-w, w + 1)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], np.float64)


def tap_tables(tw, darker):
    """(gp, gm) in Float64 and the two float32 tables: row[c][k] = float32(g±[k]); col[c][k] = float32(s·g₊[k]), float32(−s·g₋[k])
    with s = ±1/255 formed once in Float64 — a product with s, not a division by 255."""
    sg = sigma_of(tw)
    l = kernel_len(sg)
    gp, gm = gaussian_1d(sg, l), gaussian_1d(sg * math.sqrt(2.0), l)
    s = (-1.0 if darker else 1.0) / 255.0
    row = np.stack([gp.astype(np.float32), gm.astype(np.float32)])
    col = np.stack([(s * gp).astype(np.float32), (-s * gm).astype(np.float32)])
    return gp, gm, row, col


# ---- the DC level (dog_kernels.hpp, dc_sample_sum / dc_from_sum): integer arithmetic ----
def dc_level(tile, fill):
    """tile: the window's padded tile (n1 + l − 1 rows, n2 + l − 1 columns, fill already in place).  A 32 × 32 sample grid,
    the rounded mean (sum + 512) >> 10, and the fill itself when the mean lies within 8 of it."""
    tH, tW = tile.shape
    ii = (np.arange(32, dtype=np.int64) * tH) >> 5
    jj = (np.arange(32, dtype=np.int64) * tW) >> 5
    total = int(tile[np.ix_(ii, jj)].astype(np.int64).sum())
    dc = (total + 512) >> 10
    return int(fill) if abs(dc - int(fill)) <= 8 else dc


def window_tile(frame, fill, l, radii, guess):
    """The padded tile the kernels read for a 1-based guess: PaddedView fill outside the frame (src/PawsomeTracker.jl:48)."""
    hw, (r1, r2) = l >> 1, radii
    th, tw_ = 2 * r1 + 1 + 2 * hw, 2 * r2 + 1 + 2 * hw
    i0, j0 = int(guess[0]) - r1 - hw - 1, int(guess[1]) - r2 - hw - 1
    tile = np.full((th, tw_), fill, np.uint8)
    a0, a1 = max(0, -i0), min(th, frame.shape[0] - i0)
    b0, b1 = max(0, -j0), min(tw_, frame.shape[1] - j0)
    if a1 > a0 and b1 > b0:
        tile[a0:a1, b0:b1] = frame[i0 + a0:i0 + a1, j0 + b0:j0 + b1]
    return tile


# ---- the orders ----
def twopass_ring(P, Ublk):
    """dog_twopass.hpp: register-ring slots = taps per trip."""
    return ((P + 2 * Ublk - 1 + Ublk - 1) // Ublk) * Ublk


def pick_h1_outputs(n2):
    """Outputs per task of the two-pass row pass (pawsome_dog.hip), as test_seeded_fuzz_two_pass_task_sizes_vs_oracle states it."""
    return 13 if n2 / (-(-n2 // 208) * 208) > n2 / (-(-n2 // 144) * 144) + 0.05 else 9


def pick_hpass_outputs(n1):
    return 9 if n1 / (-(-n1 // 288) * 288) > n1 / (-(-n1 // 224) * 224) + 0.05 else 7


def _sym_terms(l):
    H = l >> 1
    return [(k, (k, l - 1 - k)) for k in range(H)] + [(H, (H,))]   # symmetric pairs from the edge inwards, centre last


def order(family, l, n1=None, n2=None, h1_u=4, hp_u=8, hr16=False, ph1=None, php=None):
    """The operation order of one kernel family at kernel length l.  The two-pass family needs the window shape from
    l = TWOPASS_FLUSH_L on: the chains are one trip of the register ring long, and the ring follows the outputs per task."""
    H = l >> 1
    if family == "roll":          # dog_roll.hpp: roll_row_pass; roll_col_body, dog_thin_kernel, fold_column_peak
        return dict(row=[_sym_terms(l)], col=[list(range(l))], flush=False, col_mode="interleaved")
    if family == "ring":          # dog_kernels.hpp: fir_sliding / row_block, col_block — plain chains over the l taps
        return dict(row=[[(k, (k,)) for k in range(l)]], col=[list(range(l))], flush=False, col_mode="separate")
    if family in ("fused", "tiled") or (family == "twopass" and l < TWOPASS_FLUSH_L):
        return dict(row=[_sym_terms(l)], col=[list(range(l))], flush=False, col_mode="separate")
    assert family == "twopass", family
    ph1 = ph1 or pick_h1_outputs(n2)
    php = php or pick_hpass_outputs(n1)
    # row pass (h1_block, FLUSH): whole blocks of h1_u pairs, a trip of the ring = m_r pairs; after every whole trip the chain
    # joins the total; the remaining blocks, the remaining pairs and the centre are the last chain
    terms = _sym_terms(l)
    m_r = twopass_ring(ph1, h1_u)
    full = ((H // h1_u) // (m_r // h1_u))
    row = [terms[c * m_r:(c + 1) * m_r] for c in range(full)] + [terms[full * m_r:]]
    if hr16:                      # the 16-row column form, dog_hpass_kernel<13, 16>: a plain chain (no blocked instance exists)
        return dict(row=row, col=[list(range(l))], flush=True, col_flush=False, col_mode="separate")
    # column pass (hpass_block, FLUSH): whole blocks of hp_u taps over a table that ends in zeros (a zero tap adds 0 exactly and
    # is left out here), a trip = m_c taps; the blocks after the last whole trip are the last chain — which may be empty
    m_c = twopass_ring(php, hp_u)
    fullc = (-(-l // hp_u)) // (m_c // hp_u)
    col = [list(range(c * m_c, min((c + 1) * m_c, l))) for c in range(fullc)] + [list(range(min(fullc * m_c, l), l))]
    return dict(row=row, col=col, flush=True, col_mode="separate")


# ---- float32 steps ----
def fma32(a, b, c):
    """fl32(a·b + c), one rounding."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)   # exact
    c = np.asarray(c, np.float32).astype(np.float64)
    t = p + c
    bb = t - p
    e = (p - (t - bb)) + (c - bb)                                   # TwoSum: p + c = t + e exactly
    tie = ((t.view(np.int64) & 0x1FFFFFFF) == 0x10000000) & (e != 0)  # t halfway between two float32, the exact sum not
    if tie.any():
        t = np.where(tie, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def _run_chains(chains, flush, shape, step):
    """step(acc, term) -> acc.  One chain from zero, or chains from zero added into a total from zero."""
    total = None
    for chain in chains:
        acc = np.zeros(shape, np.float32)
        for term in chain:
            acc = step(acc, term)
        if not flush:
            assert len(chains) == 1
            return acc
        total = acc if total is None else total + acc               # float32 + float32: one rounding (0 + chain is exact)
    return total


def response_f32(tile_u8, fill, tw, darker, family, n1=None, n2=None, dc=None, **geo):
    """The float32 response map (n1 × n2) of `family` for the window whose padded tile is tile_u8 (dc: the DC level, by
    default what dc_level decides)."""
    l = kernel_len(sigma_of(tw))
    tile = np.asarray(tile_u8)
    n1 = tile.shape[0] - l + 1 if n1 is None else n1
    n2 = tile.shape[1] - l + 1 if n2 is None else n2
    return response_of_order(tile, fill, tw, darker, order(family, l, n1=n1, n2=n2, **geo), dc=dc)


def response_of_order(tile_u8, fill, tw, darker, o, dc=None):
    """The float32 response map an order description `o` gives."""
    gp, gm, trow, tcol = tap_tables(tw, darker)
    l = len(gp)
    tile = np.asarray(tile_u8)
    n1, n2 = tile.shape[0] - l + 1, tile.shape[1] - l + 1
    dc = dc_level(tile, fill) if dc is None else dc
    v = (tile.astype(np.int32) - dc).astype(np.float32)             # exact integers
    NA = n1 + l - 1

    def row_step(c):
        def step(acc, term):
            k, offs = term
            s = v[:, offs[0]:offs[0] + n2]
            for off in offs[1:]:
                s = s + v[:, off:off + n2]                          # exact
            return fma32(s, trow[c, k], acc)
        return step
    R = [_run_chains(o["row"], o["flush"], (NA, n2), row_step(c)) for c in (0, 1)]
    if o["col_mode"] == "interleaved":
        acc = np.zeros((n1, n2), np.float32)
        for t in o["col"][0]:
            acc = fma32(R[0][t:t + n1], tcol[0, t], acc)            # (the kernels' first term is a multiply: the same value)
            acc = fma32(R[1][t:t + n1], tcol[1, t], acc)
        return acc
    cflush = o.get("col_flush", o["flush"])
    D = [_run_chains(o["col"], cflush, (n1, n2), lambda acc, t, c=c: fma32(R[c][t:t + n1], tcol[c, t], acc)) for c in (0, 1)]
    return D[0] + D[1]


# ---- the error-bound factor of an order (pdog_math.cpp:50-62) ----
def _chains_weight(chains, flush, weight):
    """Σ_i W_i over every rounded step: per FMA the chain's cumulative weight from zero, per addition of a chain's sum the
    total's weight after it."""
    F, total = 0.0, 0.0
    for chain in chains:
        w = 0.0
        for term in chain:
            w += weight(term)
            F += w
        if flush:
            total += w
            F += total
    return F


def factor(o, gp, gm):
    """δ = u·(V/255)·F: Σ W_i in the order `o` adds its terms, + 1 per rounded tap table (two per pass), + 2 for the final
    addition of the two channels where they keep separate chains."""
    F = 0.0
    for g in (gp, gm):
        F += _chains_weight(o["row"], o["flush"], lambda term: len(term[1]) * g[term[0]]) + 1.0
    if o["col_mode"] == "interleaved":
        W = 0.0
        for t in o["col"][0]:
            W += gp[t]
            F += W      # after the + term of tap t
            W += gm[t]
            F += W      # after the − term
        return F + 2.0
    for g in (gp, gm):
        F += _chains_weight(o["col"], o.get("col_flush", o["flush"]), lambda t: g[t]) + 1.0
    return F + 2.0


def threshold_f32(F):
    """2δ for |pixel − dc| ≤ 255 as exact_ctl rounds it, before its nextafter."""
    return np.float32(2.0 * U * F * 1.02 + 2e-9)
