"""Padding-only sub-chunks of the roll kernels (csrc/dog_roll.hpp, "padding rows"): 8 tile rows of a strip that lie outside the
frame skip staging, row pass and column FMAs when the window's DC level equals the fill.  The skip must not move a bit.

Every map case runs the same pinned roll instance with `no_pad_skip` 0 and 1 through BatchTracker.detect(..., want_resp=True):
  * the two response maps are equal as int32 views (sign of zero included);
  * each equals tests/fp32_restatement.py's float32 emulation of the roll order (np.array_equal);
  * the positions, exact mode on, equal the dense Float64 oracle's.
Content: 0/255 noise, fill 128 passed explicitly (no step edge as in test_gpu_fp32_order._scene: a flat region would move the
DC level off the fill, and the skip only exists for dc == fill — each case asserts that its DC level is the fill).  Frame
120 × 200; window heights 21 and 61; widths 45 (a partial strip), 65 (a single remainder column; also under `no_fold` and
`fold_always`, where the positions of a launch without the map are compared too: only that launch folds), 131 (two strips
plus thin columns).  Guess rows: ≥ 16 tile rows above the frame, ≥ 16 below, exactly 7 outside (no sub-chunk skipped), exactly
8 (one skipped); a 40-row frame under the 61-row window (padding at both ends).  Guess columns: −30 with width 131 at l = 65
(strip 0 wholly outside), its mirror image on the right, and — the range check keeps the last of TWO strips from ever lying
wholly right of the frame — a 195-wide window whose third strip does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 128
VARIANTS = [(100, 65), (117, 17), (201, 101)]   # l = 65 and 17: three waves per SIMD; l = 101: two


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


def _noise(fh, fw, seed, levels=(0, 255)):
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, (fh, fw)) == 1, levels[1], levels[0]).astype(np.uint8)


def _row_guess(ti0, l, ws):
    """The guess row that puts tile row 0 on (0-based) frame row ti0."""
    return ti0 + ws[0] // 2 + 1 + l // 2


def _col_guess(wj0, l, ws):
    return wj0 + ws[1] // 2 + 1 + l // 2


def _legal(g, l, fh, fw):
    hw = l // 2
    return -hw <= g[0] <= fh + hw + 1 and -hw <= g[1] <= fw + hw + 1


_EXPECT = {}


def _expected(oracle, frame, fill, l, ws, guesses):
    """Emulated maps, dense-oracle positions and DC levels of the guesses: computed once per case, shared by its launches."""
    key = (frame.tobytes(), fill, l, ws, guesses.tobytes())
    if key not in _EXPECT:
        _EXPECT.clear()
        tw, darker, radii = _tw_for_kernel_len(l), (l // 4) % 2 == 0, (ws[0] // 2, ws[1] // 2)
        K = oracle.dog_kernel(oracle.sigma(tw), darker)
        o = fr.order("roll", l, n1=2 * radii[0] + 1, n2=2 * radii[1] + 1)
        exp, pos, dcs = [], [], []
        for g in guesses:
            tile = fr.window_tile(frame, fill, l, radii, g)
            dc = fr.dc_level(tile, fill)
            dcs.append(dc)
            exp.append(fr.response_of_order(tile, fill, tw, darker, o, dc=dc))
            pos.append(tuple(int(v) for v in oracle.detect(frame, fill, K, radii, (int(g[0]), int(g[1])))))
        _EXPECT[key] = (exp, pos, dcs)
    return _EXPECT[key]


def _launch(pt, frame, fill, vid, l, ws, guesses, no_pad_skip, tuning=(), want_resp=True):
    import torch
    fh, fw = frame.shape
    bt = pt.BatchTracker(fh, fw, _tw_for_kernel_len(l), ws, (l // 4) % 2 == 0, fill)
    try:
        assert bt.info().kernel_len == l
        bt.set_variant(vid)
        for key in tuning:
            bt.set_tuning(key, 1)
        bt.set_tuning("no_pad_skip", no_pad_skip)
        bt.set_exact(1)
        assert bt.kernel_for_batch(len(guesses)) == vid
        d_f = torch.from_numpy(frame[None]).cuda()
        d_g = torch.from_numpy(np.ascontiguousarray(guesses)).cuda()
        d_fi = torch.zeros(len(guesses), dtype=torch.int32).cuda()
        if want_resp:
            pos, resp = bt.detect(d_f, d_g, d_fi, want_resp=True)
            bt.sync()
            return pos.cpu().numpy(), resp.cpu().numpy()
        pos = bt.detect(d_f, d_g, d_fi)
        bt.sync()
        return pos.cpu().numpy(), None
    finally:
        bt.close()


def _check(pt, oracle, frame, fill, vid, l, ws, guesses, tuning=(), dc_is_fill=True):
    guesses = np.asarray(guesses, np.int32)
    fh, fw = frame.shape
    assert all(_legal(g, l, fh, fw) for g in guesses), guesses
    exp, ref_pos, dcs = _expected(oracle, frame, fill, l, ws, guesses)
    assert all((dc == fill) == dc_is_fill for dc in dcs), (dcs, fill)        # the skip engages in every window / in none
    got = [_launch(pt, frame, fill, vid, l, ws, guesses, nps, tuning) for nps in (0, 1)]
    what = (vid, l, ws, tuple(tuning))
    assert np.array_equal(got[0][1].view(np.int32), got[1][1].view(np.int32)), what
    for nps in (0, 1):
        pos, resp = got[nps]
        for b, g in enumerate(guesses):
            m = np.ascontiguousarray(resp[b].T)
            assert np.array_equal(m, exp[b]), (what, nps, tuple(g))
            assert tuple(int(v) for v in pos[b]) == ref_pos[b], (what, nps, tuple(g))
    if tuning:   # the folding launch is the one without the map
        for nps in (0, 1):
            pos, _ = _launch(pt, frame, fill, vid, l, ws, guesses, nps, tuning, want_resp=False)
            assert [tuple(int(v) for v in p) for p in pos] == ref_pos, (what, nps, "no map")
    return got


def _row_guesses(l, ws, fh, fw):
    NA = ws[0] + l - 1
    col = _col_guess(3, l, ws) if ws[1] + l - 1 + 3 <= fw else fw // 2    # columns inside the frame where the tile fits
    ti0s = [-19, fh - NA + 21, -7, -8]                                     # ≥ 16 rows above, ≥ 16 below, exactly 7, exactly 8
    return [(_row_guess(t, l, ws), col) for t in ti0s]


@pytest.mark.parametrize("width", [45, 65, 131])
@pytest.mark.parametrize("height", [21, 61])
@pytest.mark.parametrize("vid,l", VARIANTS)
def test_rows_outside_the_frame(pt, oracle, vid, l, height, width):
    ws, fh, fw = (height, width), 120, 200
    frame = _noise(fh, fw, [l, height, width])
    guesses = _row_guesses(l, ws, fh, fw)
    _check(pt, oracle, frame, FILL, vid, l, ws, guesses)
    if width == 65:
        for sw in ("no_fold", "fold_always"):
            _check(pt, oracle, frame, FILL, vid, l, ws, guesses, tuning=(sw,))


@pytest.mark.parametrize("width", [45, 65, 131])
@pytest.mark.parametrize("vid,l", VARIANTS)
def test_short_frame_padding_at_both_ends(pt, oracle, vid, l, width):
    """A 40-row frame under the 61-row window: padding rows above and below, the in-frame rows in the middle."""
    ws, fh, fw = (61, width), 40, 200
    NA = ws[0] + l - 1
    frame = _noise(fh, fw, [l, 40, width])
    ti0 = -((NA - fh) // 2)
    assert -ti0 >= 8 and ti0 + NA - fh >= 8
    _check(pt, oracle, frame, FILL, vid, l, ws, [(_row_guess(ti0, l, ws), fw // 2), (_row_guess(ti0 - 5, l, ws), fw // 2 + 7)])


def test_strip_wholly_left_of_the_frame_and_its_mirror(pt, oracle):
    """Width 131, l = 65, guess column −30: the tile starts at frame column −128 and strip 0's 128 staged columns are all padding.
    The mirror image (column fw + 31) leaves three columns of strip 1 inside the frame: no strip is skipped there."""
    l, ws, fh, fw = 65, (61, 131), 120, 200
    frame = _noise(fh, fw, [l, 131, 1])
    assert _col_guess(-128, l, ws) == -30
    guesses = [(60, -30), (60, fw + 31), (_row_guess(-19, l, ws), -30), (_row_guess(fh - (61 + l - 1) + 21, l, ws), fw + 31)]
    _check(pt, oracle, frame, FILL, 100, l, ws, guesses)


@pytest.mark.parametrize("vid,l", [(100, 65), (117, 17)])
def test_last_of_three_strips_wholly_right_of_the_frame(pt, oracle, vid, l):
    """Width 195 = 3 · 64 + 3: the third strip starts at window column 128; with the tile's column 0 on frame column fw − 128 or
    beyond it reads padding only.  (The range check allows tile starts up to fw − 97.)"""
    ws, fh, fw = (21, 195), 120, 200
    frame = _noise(fh, fw, [l, 195, 2])
    guesses = [(60, _col_guess(fw - 128, l, ws)), (60, _col_guess(fw - 100, l, ws)), (_row_guess(-8, l, ws), _col_guess(fw - 128, l, ws))]
    _check(pt, oracle, frame, FILL, vid, l, ws, guesses)


@pytest.mark.parametrize("vid,l", VARIANTS)
def test_all_fill_frame(pt, oracle, vid, l):
    """Every input is the fill: every response is +0 under both settings, bit for bit."""
    ws, fh, fw = (61, 131), 120, 200
    frame = np.full((fh, fw), FILL, np.uint8)
    guesses = np.array([(60, 100), (_row_guess(-19, l, ws), 100), (-(l // 2), -(l // 2)), (fh + l // 2 + 1, fw + l // 2 + 1)], np.int32)
    for nps, (_, resp) in enumerate(_check(pt, oracle, frame, FILL, vid, l, ws, guesses)):
        assert not resp.view(np.int32).any(), (vid, nps)


def test_local_dc_scene_keeps_the_full_path(pt, oracle):
    """Levels 25 / 55 under fill 200: the DC level is not the fill, the skip must not engage, and the maps equal the emulation
    as before."""
    l, ws, fh, fw = 65, (61, 69), 120, 200
    frame = _noise(fh, fw, [l, 61, 69, 200], levels=(25, 55))
    _check(pt, oracle, frame, 200, 100, l, ws, _row_guesses(l, ws, fh, fw), dc_is_fill=False)


def test_chain_walks_into_the_top_border(pt, oracle):
    """12 frames of 100 × 100, 45-pixel-wide strips, the roll chain kernel pinned: the target walks into the top border, so more
    and more of the tile's first sub-chunks are padding.  Both settings give the oracle's chain."""
    import torch
    from oracle import synth
    from oracle.dog_oracle import OracleTracker
    h = w = 100
    tw, ws, nf = 25, (45, 45), 12
    rng = np.random.default_rng(12)
    rows = [48 - 4 * k for k in range(nf)]                      # 48 … 4
    clip = np.stack([synth.disc_frame(h, w, (r, 50 + (k % 3)), tw, True) for k, r in enumerate(rows)])
    clip = np.clip(clip.astype(np.int16) + rng.integers(-3, 4, clip.shape), 0, 255).astype(np.uint8)
    fill = oracle.mode_u8(clip[0])
    start = (rows[0] + 3, 47)
    ot = OracleTracker(clip[0], tw, ws, True, oracle)
    ot.fill = fill
    ref, g = [], start
    for f in clip:
        ot.data[...] = f
        g = ot(g)
        ref.append(tuple(int(v) for v in g))
    assert ref[-1][0] <= 8                                      # the chain did reach the border
    outs = []
    for nps in (0, 1):
        bt = pt.BatchTracker(h, w, tw, ws, True, fill)
        try:
            assert bt.info().variant == 100
            bt.set_variant(100)                                 # the persistent roll chain kernel
            bt.set_tuning("no_pad_skip", nps)
            out = bt.detect_chains(torch.from_numpy(clip).cuda().unsqueeze(0), torch.tensor([start], dtype=torch.int32).cuda())
            bt.sync()
            outs.append([tuple(int(v) for v in p) for p in out.cpu().numpy()[0]])
        finally:
            bt.close()
    assert outs[0] == outs[1]
    assert outs[0] == ref


def test_noise_windows_over_all_four_edges_exact(pt, oracle):
    """64 windows of low-amplitude noise hanging over all four edges, exact mode on: the positions are the dense oracle's,
    refined windows included (the refinement rescans the columns the strips' masks name)."""
    import torch
    l, vid, ws, fh, fw = 65, 100, (45, 131), 120, 200
    tw, hw = _tw_for_kernel_len(l), l // 2
    rng = np.random.default_rng(64)
    frame = rng.integers(FILL - 1, FILL + 2, (fh, fw)).astype(np.uint8)
    frame[rng.random((fh, fw)) < 0.9] = FILL                    # mostly flat: near-ties between the sparse speckles
    g = []
    for k in range(16):
        g += [(-hw + k, 10 + 12 * k), (fh + hw + 1 - k, 12 * k), (8 * k, -hw + k), (120 - 7 * k, fw + hw + 1 - k)]
    guesses = np.array(g, np.int32)
    assert len(guesses) == 64 and all(_legal(q, l, fh, fw) for q in guesses)
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    ref = oracle.detect_batch(np.repeat(frame[None], 64, 0), FILL, K, (ws[0] // 2, ws[1] // 2), guesses)
    for nps in (0, 1):
        bt = pt.BatchTracker(fh, fw, tw, ws, True, FILL)
        try:
            bt.set_variant(vid)
            bt.set_tuning("no_pad_skip", nps)
            bt.set_exact(1)
            out = bt.detect(torch.from_numpy(frame[None]).cuda(), torch.from_numpy(guesses).cuda(), torch.zeros(64, dtype=torch.int32).cuda())
            bt.sync()
            print("pad rows, 64 noise windows: no_pad_skip", nps, "windows refined", bt.exact_stats()[2])
            assert np.array_equal(out.cpu().numpy(), ref), nps
        finally:
            bt.close()
