"""Each kernel family's FP32 operation order, pinned bit for bit.

Exact mode's guarantee (csrc/dog_exact.hpp) rests on one premise: every kernel family adds its FP32 terms in a known order,
and the error bound δ = u·(V/255)·F·1.02 follows from that order.  tests/fp32_restatement.py states each order once, as data;
here every family runs with its kernel pinned and its response map must EQUAL the float32 emulation of that description:
  (a) np.array_equal(resp, response_f32(...)) — a reassociation, another pairing, another chain split, a change in how the
      taps or the DC level are formed, or a compiler that contracts differently fails it;
  (b) max|resp − dense Float64 oracle| ≤ δ = T/2·V/255, T the library's threshold (exact_stats) under the same pinned variant,
      V = max|pixel − dc| over the window's padded tile;
  (c) float32(2u·F·1.02 + 2e-9) ≤ T with F derived from the order that (a) has just shown the kernel to use.
Two windows per case through BatchTracker.detect(..., want_resp=True): one inside the frame, one hanging over its top-left
corner so that the fill enters the tile.  Content: 0/255 noise with a step edge, fill 128 passed explicitly (the two local-dc
cases: levels around 40, fill 200).  Every case prints one `census` line (profiles/fp32_order_census.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

pytestmark = pytest.mark.gpu

# Shapes a pinned variant refuses (pdog_set_variant fails), with the reason.  Only the fused family may appear: its tile and
# its transposed row-pass result must fit LDS together (fused_lds_bytes, 159 KB).
REFUSED = {
    (65, (45, 97)): "tile 109 x 161 f32 (78 KB) + row-pass result 97 x 139 f2 (108 KB) exceed LDS",
    (101, (45, 97)): "tile 145 x 197 f32 (125 KB) + row-pass result 97 x 175 f2 (136 KB) exceed LDS",
}


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


_SCENES = {}


def _scene(oracle, order_family, l, ws, fill, levels):
    """Frame, the two guesses and — once per (order, l, window, content) — the emulated maps, the dense references, V and F."""
    key = (order_family, l, ws, fill, levels)
    if key in _SCENES:
        return _SCENES[key]
    tw = _tw_for_kernel_len(l)
    darker = (l // 4) % 2 == 0
    radii = (ws[0] // 2, ws[1] // 2)
    n1, n2, hw = 2 * radii[0] + 1, 2 * radii[1] + 1, l // 2
    fh, fw = n1 + l - 1 + 16, n2 + l - 1 + 16
    rng = np.random.default_rng([l, ws[0], ws[1], fill])
    lo, hi = levels
    frame = np.where(rng.integers(0, 2, (fh, fw)) == 1, hi, lo).astype(np.uint8)
    frame[fh // 3:, 2 * fw // 3:] = hi                          # the step edge: noise | flat, crossing both windows' reach
    frame[:fh // 3, 2 * fw // 3:] = lo
    guesses = np.array([[radii[0] + hw + 9, radii[1] + hw + 9], [3, 5]], np.int32)   # inside the frame; over its top-left corner
    K = oracle.dog_kernel(oracle.sigma(tw), darker)
    gp, gm, _, _ = fr.tap_tables(tw, darker)
    assert len(gp) == l and K.shape[0] == l
    o = fr.order(order_family, l, n1=n1, n2=n2)
    sc = dict(tw=tw, darker=darker, frame=frame, guesses=guesses, F=fr.factor(o, gp, gm), exp=[], ref=[], V=[], dc=[])
    for g in guesses:
        tile = fr.window_tile(frame, fill, l, radii, g)
        dc = fr.dc_level(tile, fill)
        sc["dc"].append(dc)
        sc["V"].append(int(np.abs(tile.astype(np.int32) - dc).max()))
        sc["exp"].append(fr.response_of_order(tile, fill, tw, darker, o, dc=dc))
        sc["ref"].append(oracle.detect(frame, fill, K, radii, (int(g[0]), int(g[1])), want_resp=True)[1])
    assert (fr.window_tile(frame, fill, l, radii, guesses[1]) == fill).any() and not (guesses[0] - np.array(radii) - hw - 1 < 0).any()
    _SCENES.clear()                                             # (one scene at a time: the forms of a shape follow each other)
    _SCENES[key] = sc
    return sc


def _ulps(a, b):
    def lin(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(lin(np.ascontiguousarray(a)) - lin(np.ascontiguousarray(b))).max())


def _run(pt, oracle, family, l, ws, variant=None, n=2, tuning=(), fill=128, levels=(0, 255), kernel=None, order_family=None):
    """One launch; (a), (b), (c) on the two windows.  variant None: the tracker's own choice (`kernel` then says which path a
    batch of n must take).  Returns False when the variant refuses the shape."""
    import torch
    sc = _scene(oracle, order_family or family, l, ws, fill, levels)
    fh, fw = sc["frame"].shape
    bt = pt.BatchTracker(fh, fw, sc["tw"], ws, sc["darker"], fill)
    try:
        assert bt.info().kernel_len == l
        if variant is not None:
            try:
                bt.set_variant(variant)
            except pt.PdogError:
                assert family == "fused" and (l, ws) in REFUSED, (family, l, ws, variant)
                return False
        assert (l, ws) not in REFUSED or family != "fused", (l, ws)
        for key in tuning:
            bt.set_tuning(key, 1)
        if kernel is not None:
            assert bt.kernel_for_batch(n) == kernel, (family, l, ws, n, bt.kernel_for_batch(n))
        T = bt.exact_stats()[1]
        d_f = torch.from_numpy(sc["frame"][None]).cuda()
        d_fi = torch.zeros(n, dtype=torch.int32).cuda()
        batches = []
        for idx in ([np.arange(n) % 2] if n >= 2 else [np.array([0]), np.array([1])]):   # (n = 1: a launch per window)
            d_g = torch.from_numpy(np.ascontiguousarray(sc["guesses"][idx])).cuda()
            _, r = bt.detect(d_f, d_g, d_fi, want_resp=True)
            bt.sync()
            batches.append(r.cpu().numpy())
        resp = np.concatenate(batches)
    finally:
        bt.close()
    what = (family, l, ws, variant, n, tuple(tuning))
    for b in range(len(resp)):                                   # the batch's other windows repeat the two: the same bits
        assert np.array_equal(resp[b], resp[b % 2]), (what, b)
    Tf = np.float32(T)
    F_lib = (T - 2e-9) / (2.0 * fr.U * 1.02)
    for b in range(2):
        got = np.ascontiguousarray(resp[b].T)
        err = float(np.abs(got.astype(np.float64) - sc["ref"][b]).max())
        delta = T / 2.0 * sc["V"][b] / 255.0
        equal = np.array_equal(got, sc["exp"][b])
        print(f"census {family:8s} l={l:3d} {ws[0]}x{ws[1]} variant={variant} n={n} {'+'.join(tuning) or '-'} fill={fill} window={b} dc={sc['dc'][b]} V={sc['V'][b]} "
              f"bit-equal={equal} ulps={_ulps(got, sc['exp'][b])} err/delta={err / delta:.4f} F(order)={sc['F']:.2f} F(library)={F_lib:.2f}")
        assert equal, (what, b, "max distance in ulps", _ulps(got, sc["exp"][b]))                      # (a)
        assert err <= delta, (what, b, err, delta)                                                     # (b)
    assert fr.threshold_f32(sc["F"]) <= Tf, (what, sc["F"], F_lib)                                     # (c)
    return True


# ---- roll: dog_roll_kernel, dog_thin_kernel ----
@pytest.mark.parametrize("height", [21, 61, 71])
@pytest.mark.parametrize("l", [17, 65, 81, 85, 101, 149])
def test_roll_order(pt, oracle, l, height):
    """Widths: 45 a partial strip, 65 a single remainder column, 69 thin remainder columns, 71 an overlapping last strip,
    131 two strips plus thin columns.  Heights 21 / 61 / 71: fewer rows than most of these kernels have taps; four rows fewer
    and six more than l = 65.
    l = 65 folds a single remainder column into the last strip when no response map is asked for (dog_roll.hpp); with the
    map the column stays with dog_thin_kernel, which `no_fold` and `fold_always` must both leave bit-identical."""
    vid = 100 if l == 65 else 100 + l
    for width in (45, 65, 69, 71, 131):
        assert _run(pt, oracle, "roll", l, (height, width), variant=vid, kernel=vid)
        if l == 65 and width == 65:
            for sw in ("no_fold", "fold_always"):
                assert _run(pt, oracle, "roll", l, (height, width), variant=vid, kernel=vid, tuning=(sw,))


# ---- ring: dog_window_kernel ----
@pytest.mark.parametrize("ws", [(45, 45), (33, 71)])
@pytest.mark.parametrize("variant,l", [(0, 65), (1, 65), (2, 65), (10, 65), (13, 65), (20, 29)])
def test_ring_order(pt, oracle, variant, l, ws):
    assert _run(pt, oracle, "ring", l, ws, variant=variant, kernel=variant)


# ---- fused: dog_fused_kernel, compile-time-length and runtime-length instances ----
@pytest.mark.parametrize("l", [29, 65, 101])
def test_fused_order(pt, oracle, l):
    ran = 0
    for ws in ((45, 45), (45, 97)):
        for tuning in ((), ("no_fused_c",)):
            ok = _run(pt, oracle, "fused", l, ws, variant=300, kernel=300, tuning=tuning)
            assert ok == ((l, ws) not in REFUSED)
            ran += ok
    assert ran >= 2                                              # every kernel length runs, with and without the compile-time instance


# ---- tiled: dog_tiled_kernel, the tracker's own choice for one or two windows too large for the fused kernel ----
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("ws", [(129, 129), (161, 301)])
def test_tiled_order(pt, oracle, ws, n):
    assert _run(pt, oracle, "tiled", 65, ws, n=n, kernel=400)


# ---- two-pass: dog_h1_kernel + dog_hpass_kernel ----
TWOPASS_PLAIN = [(29, (45, 45)), (65, (45, 45)), (65, (61, 75))]
# The blocked cases.  61 × 75, 150 × 150, 215 × 290 (l = 101, 125) and 33 × 41 (l = 293) pick 9 / 7 and 13 / 7 outputs per task
# only; 250 × 75 and 250 × 150 add 9 / 9 and 13 / 9, and l = 113 the column pass whose last whole trip ends in the tap
# table's zero padding (its last chain is empty).
TWOPASS_BLOCKED = ([(l, ws) for l in (101, 125) for ws in ((61, 75), (150, 150), (215, 290))] +
                   [(293, (33, 41)), (101, (250, 75)), (101, (250, 150)), (113, (33, 41))])


@pytest.mark.parametrize("l,ws", TWOPASS_PLAIN + TWOPASS_BLOCKED)
def test_twopass_order(pt, oracle, l, ws):
    """n = 2: the small-batch form (DC level inside the row pass); n = 20: the four-launch form; `twopass_4l`: that form for
    two windows."""
    for n, tuning in ((2, ()), (20, ()), (2, ("twopass_4l",))):
        assert _run(pt, oracle, "twopass", l, ws, variant=200, n=n, tuning=tuning, kernel=200)


def test_twopass_blocked_cases_meet_every_task_size_pair():
    seen = {(fr.pick_h1_outputs(2 * (ws[1] // 2) + 1), fr.pick_hpass_outputs(2 * (ws[0] // 2) + 1)) for _, ws in TWOPASS_BLOCKED}
    assert seen == {(9, 7), (9, 9), (13, 7), (13, 9)}, seen


@pytest.mark.parametrize("l", [101, 113, 117, 125, 137, 293])
def test_twopass_threshold_is_the_blocked_orders(pt, l):
    """The library's two-pass threshold is the one the blocked order gives — from both sides (c alone only bounds it from
    below).  l = 113, 117, 137: a whole trip of the column pass reaches past the l taps."""
    tw, ws = _tw_for_kernel_len(l), (61, 75)
    gp, gm, _, _ = fr.tap_tables(tw, True)
    F = fr.factor(fr.order("twopass", l, n1=61, n2=75), gp, gm)
    bt = pt.BatchTracker(240, 320, tw, ws, True, 128)
    try:
        bt.set_variant(200)
        T = bt.exact_stats()[1]
    finally:
        bt.close()
    assert float(fr.threshold_f32(F)) <= T <= float(fr.threshold_f32(F)) * (1 + 1e-6), (l, F, (T - 2e-9) / (2.0 * fr.U * 1.02))


# ---- local dc: content far from the fill ----
@pytest.mark.parametrize("family,l,ws,variant", [("roll", 65, (61, 69), 100), ("twopass", 101, (61, 75), 200)])
def test_local_dc_order(pt, oracle, family, l, ws, variant):
    """Levels 25 / 55 under fill 200: the window inside the frame takes its sampled mean as the DC level, the one over the
    corner a level between content and fill — dc_level decides, and V = max|pixel − dc| over the tile."""
    sc = _scene(oracle, family, l, ws, 200, (25, 55))
    assert sc["dc"][0] != 200 and 25 <= sc["dc"][0] <= 55 and sc["dc"][1] not in (200, sc["dc"][0])
    assert _run(pt, oracle, family, l, ws, variant=variant, fill=200, levels=(25, 55), kernel=variant)
