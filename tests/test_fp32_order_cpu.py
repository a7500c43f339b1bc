"""The FP32 operation orders of the kernel families (tests/fp32_restatement.py) against the dense Float64 oracle, on the CPU:
every order's error stays inside the bound its OWN factor gives — δ = u·F·V/255 with no slack — and the factors derived from
the order descriptions are the documented ones (csrc/dog_exact.hpp, csrc/pdog_math.cpp).  That the kernels really use these
orders is tests/test_gpu_fp32_order.py's part.

`python tests/test_fp32_order_cpu.py` rewrites the CPU section of profiles/fp32_order_census.txt."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = (45, 45)
PLAIN = [(fam, l) for fam in ("roll", "ring", "fused", "twopass") for l in (29, 65, 109) if not (fam == "twopass" and l >= fr.TWOPASS_FLUSH_L)]
BLOCKED = [("twopass", l) for l in (101, 125, 293)]
INPUTS = ("noise", "step", "diagonal", "checker", "pm1")


def tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


def make_tile(kind, l, ws=WS, seed=0):
    """(tile, V): the padded tile of a ws window at fill 128.  0/255 content has V = max|pixel − 128| = 128."""
    th, tw_ = ws[0] + l - 1, ws[1] + l - 1
    rng = np.random.default_rng([seed, l, INPUTS.index(kind)])
    ii, jj = np.mgrid[0:th, 0:tw_]
    if kind == "noise":
        t = rng.integers(0, 2, (th, tw_)) * 255
    elif kind == "step":
        t = np.where(jj < tw_ // 2, 0, 255)
    elif kind == "diagonal":
        t = np.where((2 * ii + 1 - th) * tw_ + (2 * jj + 1 - tw_) * th < 0, 0, 255)   # through the tile's centre: the sampled mean stays at the fill
    elif kind == "checker":
        t = np.where(((ii // 16) + (jj // 16)) % 2 == 0, 0, 255)
    else:
        return (128 + rng.integers(-1, 2, (th, tw_))).astype(np.uint8), 1
    return t.astype(np.uint8), 128


def dense_ref(oracle, tile, l, tw, ws=WS):
    """The oracle's dense Float64 response of the window whose padded tile is `tile` (the tile is the frame, the guess its centre)."""
    radii = (ws[0] // 2, ws[1] // 2)
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    assert K.shape[0] == l
    _, r = oracle.detect(tile, 128, K, radii, (l // 2 + radii[0] + 1, l // 2 + radii[1] + 1), want_resp=True)
    return r


def measure(oracle, fam, l, kind):
    """(err, δ, F) of one order on one input."""
    tw = tw_for_kernel_len(l)
    tile, V = make_tile(kind, l)
    assert fr.dc_level(tile, 128) == 128
    gp, gm, _, _ = fr.tap_tables(tw, True)
    F = fr.factor(fr.order(fam, l, n1=WS[0], n2=WS[1]), gp, gm)
    got = fr.response_f32(tile, 128, tw, True, fam)
    assert got.dtype == np.float32 and got.shape == WS
    err = float(np.abs(got.astype(np.float64) - dense_ref(oracle, tile, l, tw)).max())
    return err, fr.U * F * V / 255.0, F


def test_tables_are_the_oracles(oracle):
    for tw in (5, 10, 25, 40, 77.5, 120):
        s = fr.sigma_of(tw)
        assert s == oracle.sigma(tw) and fr.kernel_len(s) == oracle.kernel_len(s)
        l = fr.kernel_len(s)
        assert np.array_equal(fr.gaussian_1d(s, l), oracle.gaussian_1d(s, l))
        assert np.array_equal(fr.gaussian_1d(s * math.sqrt(2.0), l), oracle.gaussian_1d(s * math.sqrt(2.0), l))


def test_fma32_rounds_once():
    """The case a float64 detour gets wrong: (1 + 2^-23)(1 − 2^-23) + (2^24 + 2) = 2^24 + 3 − 2^-46.  Float64 rounds the sum to
    2^24 + 3, the tie between the float32 neighbours 2^24 + 2 and 2^24 + 4, and ties-to-even then gives 2^24 + 4; one rounding
    of the exact sum gives 2^24 + 2."""
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23), np.float32(2.0 ** 24 + 2)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(2.0 ** 24 + 4)
    assert fr.fma32(a, b, c) == np.float32(2.0 ** 24 + 2)
    assert fr.fma32(a, a, c) == np.float32(2.0 ** 24 + 4)          # 2^24 + 3 + 2^-22 + 2^-46: above the tie
    assert fr.fma32(np.float32(1.0), np.float32(1.0), c) == np.float32(2.0 ** 24 + 4)   # the tie itself: to even
    assert fr.fma32(np.float32(3.0), np.float32(0.5), np.float32(0.25)) == np.float32(1.75)


def test_dc_level_rule():
    t = np.full((64, 96), 40, np.uint8)
    assert fr.dc_level(t, 200) == 40 and fr.dc_level(t, 47) == 47 and fr.dc_level(t, 49) == 40
    t[::2] = 41                      # the grid's rows (2i) are all 41s
    assert fr.dc_level(t, 200) == 41


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("fam,l", PLAIN + BLOCKED)
def test_order_error_within_its_own_bound(oracle, fam, l, kind):
    err, delta, F = measure(oracle, fam, l, kind)
    print(f"{fam} l={l} {kind}: err {err:.3e} delta {delta:.3e} err/delta {err / delta:.4f} F {F:.2f}")
    assert err <= delta, (fam, l, kind, err, delta)


@pytest.mark.parametrize("kind", ["noise", "diagonal"])
def test_16_row_column_form_within_its_own_bound(oracle, kind):
    """dog_hpass_kernel<13, 16> (no default launch uses it): the blocked row pass under ONE column chain."""
    l, tw = 101, tw_for_kernel_len(101)
    tile, V = make_tile(kind, l)
    gp, gm, _, _ = fr.tap_tables(tw, True)
    o = fr.order("twopass", l, n1=WS[0], n2=WS[1], hr16=True)
    assert len(o["col"]) == 1 and len(o["row"]) > 1
    err = float(np.abs(fr.response_of_order(tile, 128, tw, True, o).astype(np.float64) - dense_ref(oracle, tile, l, tw)).max())
    assert err <= fr.U * fr.factor(o, gp, gm) * V / 255.0


def test_factors_are_the_documented_ones():
    """dog_exact.hpp / pdog_math.cpp: l = 65: 157 (roll), 94 (fused, tiled, two-pass), 138 (ring) against 6l + 4 = 394; l = 293,
    two-pass at its default geometry: 72 against 1762 — here from the order descriptions, not from the library's formulas."""
    gp, gm, _, _ = fr.tap_tables(25, True)
    assert len(gp) == 65
    F = {fam: fr.factor(fr.order(fam, 65), gp, gm) for fam in ("roll", "fused", "tiled", "ring", "twopass")}
    assert [round(F[f]) for f in ("roll", "fused", "tiled", "twopass", "ring")] == [157, 94, 94, 94, 138], F
    gp, gm, _, _ = fr.tap_tables(120, True)
    assert len(gp) == 293
    # the default geometry — 13 outputs per row-pass task, 7 per column-pass task: the tracker's defaults and what the
    # 205 × 205 window of the l = 293 configuration picks; a 45 × 45 window picks 9 / 7, shorter trips: 70
    assert (fr.pick_h1_outputs(205), fr.pick_hpass_outputs(205)) == (13, 7) and (fr.pick_h1_outputs(45), fr.pick_hpass_outputs(45)) == (9, 7)
    assert round(fr.factor(fr.order("twopass", 293, n1=205, n2=205), gp, gm)) == 72
    assert round(fr.factor(fr.order("twopass", 293, n1=45, n2=45), gp, gm)) == 70
    assert fr.factor(fr.order("twopass", 293, n1=45, n2=45, hr16=True), gp, gm) < fr.factor(fr.order("fused", 293), gp, gm)


def test_blocked_chains_cover_every_tap_once():
    """Every geometry of the blocked order: the chains partition the terms, whole trips first (l = 113, 117, 137: the column
    pass's last whole trip ends in the table's zero padding and the last chain is empty)."""
    for l in range(101, 302, 4):
        for ph1 in (9, 13):
            for php in (7, 9):
                o = fr.order("twopass", l, ph1=ph1, php=php)
                assert [t for ch in o["row"] for t in ch] == fr._sym_terms(l)
                assert [t for ch in o["col"] for t in ch] == list(range(l))
                assert all(len(ch) == fr.twopass_ring(ph1, 4) for ch in o["row"][:-1]) and len(o["row"][-1]) >= 1
                assert all(len(ch) <= fr.twopass_ring(php, 8) for ch in o["col"])
    assert fr.order("twopass", 113, ph1=9, php=7)["col"][-1] == []


def census(oracle):
    lines = []
    for fam, l in PLAIN + BLOCKED:
        for kind in INPUTS:
            err, delta, F = measure(oracle, fam, l, kind)
            lines.append(f"{fam + (' blocked' if l >= fr.TWOPASS_FLUSH_L and fam == 'twopass' else ''):16s} l={l:3d} {kind:9s} "
                         f"err {err:.3e}  delta {delta:.3e}  err/delta {err / delta:.4f}  F(order) {F:.2f}")
    return lines


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle.dog_oracle import Oracle, build
    build()
    path = os.path.join(ROOT, "profiles", "fp32_order_census.txt")
    old = open(path).read() if os.path.exists(path) else ""
    mark = "== GPU"
    tail = old[old.index(mark):] if mark in old else ""
    head = ("FP32 operation orders (tests/fp32_restatement.py) against the dense Float64 oracle.\n"
            "== CPU: float32 emulation of each order, 45 x 45 window, fill 128, delta = u * F(order) * V / 255 (no slack);\n"
            "   written by `python tests/test_fp32_order_cpu.py`, asserted by tests/test_fp32_order_cpu.py\n")
    with open(path, "w") as f:
        f.write(head + "\n".join(census(Oracle())) + "\n" + tail)
