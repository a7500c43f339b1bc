"""pdog_detect_peaks on the GPU: the K best, mutually separated peaks of a window (include/pawsome_peaks.h).

Every comparison of picks is exact.  `ij`, `peak` and `count` are held to tests/peaks_restatement.py applied to the map THE
SAME CALL returned, with pick 1 what detect() returns on the same inputs — per kernel family, pinned as
tests/test_gpu_layout.py pins them —, the list path to the no-list path, a strided view to its contiguous twin, a chunked
batch to the unchunked one, and the four-disc scenes to the Float64 oracle (tests/test_peaks_cpu.py shows without a GPU that
both arithmetics rank those alike).  The whole file fails on a library without the symbol."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_frames as lf  # noqa: E402
import peaks_restatement as pr  # noqa: E402
import peaks_scenes as ps  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 128


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_detect_peaks")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(seed, nf=5, h=H, w=W, amp=20, discs=3, rad=4):
    """Noise of +-amp around 128 (many local maxima) and a few dark discs per frame."""
    rng = np.random.default_rng(seed)
    f = (128 + rng.integers(-amp, amp + 1, (nf, h, w))).astype(np.uint8)
    yy, xx = np.ogrid[0:h, 0:w]
    for k in range(nf):
        for _ in range(discs):
            ci, cj = int(rng.integers(8, h - 8)), int(rng.integers(8, w - 8))
            f[k][(yy - ci) ** 2 + (xx - cj) ** 2 <= rad * rad] = int(rng.integers(0, 60))
    return f


def _guesses(seed, n, ws, l, beside):
    """n guesses: inside the frame, over each corner, random ones up to the reference's pad outside (l - l // 2 - 1) — and,
    where the pad allows it, one whose window lies wholly beside the frame on the column axis (its index is returned)."""
    rng = np.random.default_rng(seed)
    pad = l - l // 2 - 1
    g = [(H // 2, W // 2), (3, 4), (H - 2, W - 3), (2, W - 1), (H + min(pad, 5), 6)]
    k_beside = None
    if beside:
        assert ws[1] // 2 + 1 <= pad
        k_beside = len(g)
        g.append((H // 2 + 3, W + ws[1] // 2 + 1))
    while len(g) < n:
        g.append((int(rng.integers(1 - pad, H + pad + 1)), int(rng.integers(1 - pad, W + pad + 1))))
    return np.array(g[:n], np.int32), (k_beside if k_beside is not None and k_beside < n else None)


def _peaks(bt, d_frames, d_g, k, md, d_fi):
    ij, peak, count, resp = bt.detect_peaks(d_frames, d_g, k, md, d_fi, want_resp=True)
    bt.sync()
    return ij.cpu().numpy(), peak.cpu().numpy(), count.cpu().numpy(), resp.cpu().numpy()


def _assert_equals_restatement(bt, got, pick1, g, k, md, what):
    ij, peak, count, resp = got
    info = bt.info()
    md = pr.default_min_distance(info.target_width) if md is None else md
    wij, wpeak, wcount = pr.select_batch(resp, g, (info.radius_h, info.radius_w), (info.frame_h, info.frame_w), pick1, k, md)
    assert np.array_equal(count, wcount), (what, np.flatnonzero(count != wcount), count, wcount)
    bad = np.flatnonzero((ij != wij).reshape(len(g), -1).any(1))
    assert bad.size == 0, (what, bad, g[bad], ij[bad[0]], wij[bad[0]])
    assert np.array_equal(peak.view(np.int32), wpeak.view(np.int32)), (what, peak, wpeak)
    assert ((count >= 1) & (count <= k)).all()
    return wcount


# ---- bit-equality with the restatement, per kernel family ----
FAMILIES = [
    # name, target width, window, variant to pin (None: the tracker's own choice), kernel_for_batch, tuning, batch sizes
    ("roll l29 61", 10, (61, 61), 129, 129, (), (37, 1)),
    ("roll l29 65", 10, (65, 65), 129, 129, (), (37,)),
    ("roll l65 61", 25, (61, 61), 100, 100, (), (37, 1)),
    ("roll l65 65 thin", 25, (65, 65), 100, 100, ("no_fold",), (37,)),
    ("roll l65 65 fold", 25, (65, 65), 100, 100, ("fold_always",), (37,)),
    ("ring l29 61", 10, (61, 61), 20, 20, (), (37, 1)),
    ("ring l65 65", 25, (65, 65), 13, 13, (), (37,)),
    ("two-pass l65 61", 25, (61, 61), 200, 200, (), (37, 1)),
    ("two-pass l29 65", 10, (65, 65), 200, 200, (), (37,)),
    ("fused l29 61", 10, (61, 61), 300, 300, (), (37, 1)),
    ("fused l65 65", 25, (65, 65), 300, 300, ("no_fused_c",), (37,)),
    ("tiled l65 129", 25, (129, 129), None, 400, (), (2, 1)),
]


@pytest.mark.parametrize("name,tw,ws,variant,kernel,tuning,sizes", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_picks_equal_the_restatement(pt, name, tw, ws, variant, kernel, tuning, sizes):
    """K = 1, 3 and 32 (the last with min_distance 4, so that many picks are made; the default distance leaves count < K) over
    n = 37 windows behind a frame index and n = 1 without one: inside the frame, over its corners, up to the pad outside and —
    at l = 65 with the 61 x 61 window, where the pad allows it — wholly beside it (count == 1).  Each launch again with
    "peaks_no_list": identical outputs."""
    frames = _frames(len(name))
    d_frames = _cuda(frames)
    bt = pt.BatchTracker(H, W, tw, ws, True, 128)
    try:
        l = bt.info().kernel_len
        if variant is not None:
            bt.set_variant(variant)
        for key in tuning:
            bt.set_tuning(key, 1)
        for n in sizes:
            assert bt.kernel_for_batch(n) == kernel, (name, n, bt.kernel_for_batch(n))
            g, k_beside = _guesses(7 * n + len(name), n, ws, l, beside=(l == 65 and ws == (61, 61)))
            fi = np.random.default_rng(n).integers(0, len(frames), n).astype(np.int32) if n > 1 else None
            d_g, d_fi = _cuda(g), (None if fi is None else _cuda(fi))
            pick1 = bt.detect(d_frames, d_g, d_fi)
            bt.sync()
            pick1 = pick1.cpu().numpy()
            for k, md in ((1, None), (3, None), (32, 4), (32, None)):
                served = bt.peaks_counts()
                got = _peaks(bt, d_frames, d_g, k, md, d_fi)
                wcount = _assert_equals_restatement(bt, got, pick1, g, k, md, (name, n, k, md))
                assert np.array_equal(got[0][:, 0], pick1)
                after = bt.peaks_counts()
                assert after[0] - served[0] == n and after[1] == served[1]          # served, and no list overflowed
                if k_beside is not None:
                    assert wcount[k_beside] == 1 and got[2][k_beside] == 1
                if k == 32:
                    assert (wcount < 32).any() if md is None else wcount.max() > 8, (name, wcount)
                bt.set_tuning("peaks_no_list", 1)
                scan = _peaks(bt, d_frames, d_g, k, md, d_fi)
                bt.set_tuning("peaks_no_list", 0)
                for a, b in zip(got, scan):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, n, k, md, "no list")
    finally:
        bt.close()


# ---- pick 1 ----
@pytest.mark.parametrize("exact", [1, 0])
def test_pick_one_is_detects_position(pt, exact):
    """On a hard, noise-only batch (tests/layout_frames.py, "empty": levels 126 … 130 and 2 x 2 blocks whose four responses
    tie exactly, so exact mode refines windows) pick 1 equals detect() on the same inputs, with exact mode on and off; the
    picks still equal the restatement over the returned map."""
    sc = lf.scene("l65 45x45", "empty")
    g = np.array([q for _, q in sc.windows], np.int32)
    fi = np.array([k for k, _ in sc.windows], np.int32)
    d_frames, d_g, d_fi = _cuda(sc.frames), _cuda(g), _cuda(fi)
    bt = pt.BatchTracker(sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)
    try:
        bt.set_exact(exact)
        pick1 = bt.detect(d_frames, d_g, d_fi)
        bt.sync()
        pick1 = pick1.cpu().numpy()
        before = bt.exact_stats()[2]
        got = _peaks(bt, d_frames, d_g, 4, None, d_fi)
        refined = bt.exact_stats()[2] - before
        assert (refined > 0) == bool(exact), refined
        assert np.array_equal(got[0][:, 0], pick1)
        _assert_equals_restatement(bt, got, pick1, g, 4, None, ("hard", exact))
    finally:
        bt.close()


# ---- a list that overflows ----
def test_overflowing_list_scans_the_map(pt):
    """Noise under the shortest kernel (target width 1, l = 5) has a local maximum every eighth pixel: a 129 x 129 window
    inside the frame holds more candidates than the list.  The counter tells, the picks still equal the restatement, and
    with "peaks_no_list" the same picks come without the counter moving."""
    rng = np.random.default_rng(11)
    h = w = 160
    frames = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    g = np.array([[80, 80], [70, 90], [90, 75]], np.int32)
    d_frames, d_g = _cuda(frames), _cuda(g)
    bt = pt.BatchTracker(h, w, 1, (129, 129), True, 128)
    try:
        assert bt.info().kernel_len == 5
        pick1 = bt.detect(d_frames, d_g)
        bt.sync()
        pick1 = pick1.cpu().numpy()
        c0 = bt.peaks_counts()
        got = _peaks(bt, d_frames, d_g, 32, None, None)
        c1 = bt.peaks_counts()
        for b in range(3):
            assert pr.n_candidates(got[3][b].T, g[b], (64, 64), (h, w)) > pr.LIST_CAPACITY
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (3, 3)
        _assert_equals_restatement(bt, got, pick1, g, 32, None, "overflow")
        assert (got[2] == 32).all()
        bt.set_tuning("peaks_no_list", 1)
        scan = _peaks(bt, d_frames, d_g, 32, None, None)
        c2 = bt.peaks_counts()
        assert (c2[0] - c1[0], c2[1] - c1[1]) == (3, 0)
        for a, b in zip(got, scan):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        bt.close()


# ---- scenes against the Float64 oracle ----
@pytest.mark.parametrize("name", list(ps.SCENES))
def test_four_discs_in_contrast_order(pt, oracle, name):
    sc = ps.scene(name)
    K = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    pos, R64 = oracle.detect(sc.frame, sc.fill, K, sc.radii, sc.guess, want_resp=True)
    want, _, wcount = pr.select(R64, sc.guess, sc.radii, sc.hw, pos, 4, pr.default_min_distance(sc.tw))
    assert wcount == 4 and [tuple(p) for p in want] == [tuple(c) for c in sc.centres]
    bt = pt.BatchTracker(sc.hw[0], sc.hw[1], sc.tw, sc.ws, True, sc.fill)
    try:
        ij, peak, count = bt.detect_peaks(_cuda(sc.frame[None]), _cuda(np.array([sc.guess], np.int32)), 4)
        bt.sync()
        assert count.cpu().tolist() == [4] and np.array_equal(ij.cpu().numpy()[0], want), (name, ij.cpu().numpy())
        pk = peak.cpu().numpy()[0]
        assert (np.diff(pk) < 0).all() and pk[3] > 0
    finally:
        bt.close()


def test_two_identical_discs_come_in_column_major_order(pt):
    sc = ps.scene("twins")
    bt = pt.BatchTracker(sc.hw[0], sc.hw[1], sc.tw, sc.ws, True, sc.fill)
    try:
        for exact in (1, 0):
            bt.set_exact(exact)
            ij, peak, count = bt.detect_peaks(_cuda(sc.frame[None]), _cuda(np.array([sc.guess], np.int32)), 2)
            bt.sync()
            assert [tuple(p) for p in ij.cpu().numpy()[0]] == [(70, 50), (40, 110)] and count.cpu().tolist() == [2]
            pk = peak.cpu().numpy()[0]
            assert pk[0] == pk[1] > 0
    finally:
        bt.close()


# ---- layouts, chunks, errors ----
def test_a_strided_offset_view_gives_the_twins_outputs(pt):
    sc = lf.scene("l29 21x21", "fill")
    lay = sc.worst()
    g = np.array([q for _, q in sc.windows], np.int32)
    fi = np.array([k for k, _ in sc.windows], np.int32)
    bt = pt.BatchTracker(sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)
    try:
        twin = _peaks(bt, _cuda(sc.frames), _cuda(g), 5, 3, _cuda(fi))
        view = _peaks(bt, lf.to_device(lay), _cuda(g), 5, 3, _cuda(fi))
        for a, b in zip(twin, view):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), lay.describe()
        assert twin[2].max() > 1
    finally:
        bt.close()


_CHUNK_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import pawsometracker_jl_amd as pt
rng = np.random.default_rng(3)
H, W, n = 96, 128, 150
frames = (128 + rng.integers(-20, 21, (4, H, W))).astype(np.uint8)
g = np.stack([rng.integers(1, H + 1, n), rng.integers(1, W + 1, n)], 1).astype(np.int32)
fi = rng.integers(0, 4, n).astype(np.int32)
d = lambda a: torch.from_numpy(a).cuda()
bt = pt.BatchTracker(H, W, 10, (61, 61), True, 128)
bt.set_variant(129)                     # (pinned: a chunk's size must not choose another kernel family than the batch's)
whole = bt.detect_peaks(d(frames), d(g), 6, 4, d(fi), want_resp=True)[:3]      # the caller's buffer: one chunk
parts = bt.detect_peaks(d(frames), d(g), 6, 4, d(fi))                          # the tracker's scratch: 1 MiB holds 70 maps
bt.sync()
same = all(torch.equal(a, b) for a, b in zip(whole, parts))
plain = bt.detect_peaks(d(np.ascontiguousarray(frames[fi])), d(g), 6, 4)       # no frame index: a chunk starts at its own frame
bt.sync()
same2 = all(torch.equal(a, b) for a, b in zip(whole, plain))
print("chunked", same, same2, int(whole[2].max()), bt.peaks_counts()[0])
bt.close()
"""


def test_a_batch_in_chunks_equals_the_whole_batch():
    """PDOG_MAP_MB is read when a tracker is created: a child process with 1 MiB of map scratch serves 150 windows of
    61 x 61 (14.9 KB each) in three chunks."""
    env = dict(os.environ, PDOG_MAP_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHUNK_CHILD % ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    words = p.stdout.split()
    assert words[:3] == ["chunked", "True", "True"] and int(words[3]) > 2 and int(words[4]) == 450, p.stdout


def test_bad_arguments_launch_nothing(pt):
    """Every PDOG_E_ARG case: the status, nothing served, and the tracker works afterwards."""
    import torch
    from pawsometracker_jl_amd import _lib
    frames = _cuda(_frames(1, nf=2))
    g = _cuda(np.array([[40, 60], [50, 70]], np.int32))
    bt = pt.BatchTracker(H, W, 10, (21, 21), True, 128)
    try:
        ij = torch.zeros((2, 3, 2), dtype=torch.int32, device="cuda")
        L = pt.lib()
        P = lambda t: C.c_void_p(t.data_ptr())
        ok = dict(t=bt._h, f=P(frames), fs=frames.stride(0), rs=frames.stride(1), nf=2, fi=None, g=P(g), n=2, k=3, md=0, ij=P(ij))

        def call(**kw):
            a = dict(ok, **kw)
            return L.pdog_detect_peaks(a["t"], a["f"], a["fs"], a["rs"], a["nf"], a["fi"], a["g"], a["n"], a["k"], a["md"], a["ij"], None, None, None)

        before = bt.peaks_counts()
        for kw in (dict(t=None), dict(f=None), dict(g=None), dict(ij=None), dict(k=0), dict(k=33), dict(n=-1), dict(nf=0),
                   dict(rs=W - 1), dict(rs=_lib.PDOG_MAX_ROW_STRIDE + 1), dict(fs=-1), dict(n=3)):
            assert call(**kw) == _lib.PDOG_E_ARG, kw
            assert L.pdog_last_error() != b""
        assert bt.peaks_counts() == before and int(ij.abs().sum()) == 0
        assert call(n=0) == _lib.PDOG_OK and bt.peaks_counts() == before
        for exc, kw in ((ValueError, dict(k=0)), (ValueError, dict(k=33)), (TypeError, dict(k=2.0)), (ValueError, dict(k=2, min_distance=0)),
                        (TypeError, dict(k=2, min_distance=1.5))):
            with pytest.raises(exc):
                bt.detect_peaks(frames, g, **kw)
        with pytest.raises(TypeError):
            bt.detect_peaks(frames.cpu(), g, 2)
        with pytest.raises(ValueError):
            bt.detect_peaks(frames, g, 2, frame_index=torch.zeros(3, dtype=torch.int32, device="cuda"))
        assert bt.peaks_counts() == before
        assert call() == _lib.PDOG_OK
        bt.sync()
        assert bt.peaks_counts()[0] == before[0] + 2 and torch.equal(ij[:, 0], bt.detect(frames, g))
    finally:
        bt.close()


# ---- track_video(n_targets=…) ----
def _three_beetles():
    """60 frames of 100 x 100, background 128, three dark discs (target width 5) of values 0 / 40 / 80 that start inside the
    reference's 25 x 25 bootstrap window, 18 … 20 pixels apart, and walk away from each other at 0.3 pixels per frame."""
    nf, h, w = 60, 100, 100
    starts = np.array([(41, 41), (41, 59), (59, 50)], float)
    steps = np.array([(-0.2, -0.3), (-0.2, 0.3), (0.3, 0.0)])
    frames = np.full((nf, h, w), 128, np.uint8)
    yy, xx = np.ogrid[0:h, 0:w]
    for k in range(nf):
        for (ci, cj), v in zip(np.rint(starts + k * steps).astype(int), (0, 40, 80)):
            frames[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= 4] = v
    return frames


def test_track_video_finds_its_targets(pt, oracle):
    import torch
    frames = _three_beetles()
    tw, args = 5, dict(rate=24, start=0, stop=2.5, fps=24, target_width=5)
    # the oracle-found starts: the rule over the oracle's Float64 response of the bootstrap window (sz .÷ 4 around the centre)
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    pos, R64 = oracle.detect(frames[0], 128, K, (12, 12), (50, 50), want_resp=True)
    sij, speak, scount = pr.select(R64, (50, 50), (12, 12), (100, 100), pos, 4, pr.default_min_distance(tw))
    assert [tuple(p) for p in sij[:3]] == [(41, 41), (41, 59), (59, 50)] and (speak[:3] > 0).all()
    # nothing else in the window responds: the oracle's Float64 sums leave ~1e-16 on the flat background (its kernel's taps do
    # not cancel exactly), the kernels subtract the window's DC level first and leave exactly 0 there
    assert scount == 3 or speak[3] < 1e-12 * speak[2]
    d_frames = _cuda(frames)
    seen, seen_list = [], []
    ts, idx, sub = pt.track_video(d_frames, n_targets=3, subpixel=True, diagnostic=lambda k0, ov: seen.append((k0, ov.cpu().clone())), **args)
    locs = [("ij", (int(i), int(j))) for i, j in sij[:3]]
    ts2, idx2, sub2 = pt.track_video(d_frames, start_locations=locs, subpixel=True,
                                     diagnostic=lambda k0, ov: seen_list.append((k0, ov.cpu().clone())), **args)
    assert idx.shape == (3, 60, 2) and torch.equal(idx, idx2) and torch.equal(sub, sub2) and np.array_equal(ts, ts2)
    assert [tuple(p) for p in idx[:, 0].cpu().tolist()] == [(41, 41), (41, 59), (59, 50)]
    assert len(seen) == len(seen_list) > 0 and all(a == b and torch.equal(x, y) for (a, x), (b, y) in zip(seen, seen_list))
    ends = idx[:, -1].cpu().numpy()
    assert np.abs(ends - np.array([(29, 23), (29, 77), (77, 50)])).max() <= 2           # each chain followed its own disc
    _, idx3 = pt.track_video(d_frames, n_targets=2, min_distance=19, **args)             # (41, 59) is 18 from pick 1: suppressed
    assert [tuple(p) for p in idx3[:, 0].cpu().tolist()] == [(41, 41), (59, 50)]
    with pytest.raises(ValueError, match="only 3"):
        pt.track_video(d_frames, n_targets=4, **args)
    with pytest.raises(ValueError, match="not both"):
        pt.track_video(d_frames, n_targets=3, start_locations=locs, **args)
    _, idx1 = pt.track_video(d_frames, **args)                                           # without the keyword: the reference's one target
    assert torch.equal(idx1[0], idx[0])
