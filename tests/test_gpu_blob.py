"""pdog_blob on the GPU (blob_kernel's two tiers, BatchTracker.blobs, Tracker.blob, the track functions' shape_connectivity):
the ten integers bit for bit and the six floats to 1e-9 (the device's atan2 and hypot) against tests/blob_restatement.py — on
every scene of tests/shape_scenes.py and tests/blob_scenes.py for both connectivities, on noise at every radius 2 ... 127 (every
word boundary of the row, the tier boundary at 31 | 32, the radius at which the dynamic LDS crosses 48 KiB), on narrow frames,
clamped positions, many positions in one call; frame stacks behind other layouts held to their contiguous twins exactly; the
shapes of calls; every refusal; and the track functions' keyword.  The whole file fails on a library without the symbol."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_restatement as BR  # noqa: E402
import background_scenes as BS  # noqa: E402
import blob_restatement as BLR  # noqa: E402
import blob_scenes as BLS  # noqa: E402
import layout_frames as LF  # noqa: E402
import shape_scenes as SS  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_blob")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _close(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.abs(got[ok] - want[ok]).max(initial=0.0) <= TOL


def _run_case(pt, c, connectivity, shape_too=False):
    """One case as one call: (shape, sums) on the host side of the comparison, held to the restatement."""
    want, words = BLS.reference(c, connectivity)
    h, w = c.frames.shape[1:]
    with pt.BatchTracker(h, w, c.tw, (21, 21), c.darker, c.fill) as bt:
        d_frames, d_ij, d_fi = _cuda(c.frames), _cuda(c.ij), _cuda(c.fi)
        shp, sums = bt.blobs(d_frames, d_ij, d_fi, c.radius or None, c.min_contrast, connectivity, want_sums=True)
        plain = bt.shapes(d_frames, d_ij, d_fi, c.radius or None, c.min_contrast, want_sums=True)[1] if shape_too else None
        bt.sync()
    got = sums.cpu().numpy()
    print(c.name, connectivity, got[0].tolist())
    assert np.array_equal(got, words), (c.name, connectivity, got[(got != words).any(1)][:4].tolist(), words[(got != words).any(1)][:4].tolist())
    assert _close(shp, want), (c.name, connectivity)
    return got, plain.cpu().numpy() if shape_too else None


# ---- every scene of the shape rule ----
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", [c.name for c in SS.cases()])
def test_every_shape_scene_equals_the_restatement(pt, name, connectivity):
    got, plain = _run_case(pt, SS.case(name), connectivity, shape_too=True)
    one = got[:, 0] == got[:, 8]                  # the mask is one component there: pdog_shape's integers, bit for bit
    assert np.array_equal(got[one, :8], plain[one])
    assert np.array_equal(got[:, 6:9], plain[:, [6, 7, 0]])
    assert one.all() == (name not in ("second object R 25", "empty floor min_contrast 1"))


# ---- the blob scenes: diagonal touch, seed tie, the bar, the long geodesics in both tiers ----
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", [c.name for c in BLS.cases()])
def test_every_blob_scene_equals_the_restatement(pt, name, connectivity):
    got, _ = _run_case(pt, BLS.case(name), connectivity)
    if name == "diagonal touch":
        assert got[0, 0] == (50 if connectivity == 8 else 25)
    if name == "seed tie":
        assert got[0, 0] == 25 and got[0, 1] < 0 and got[0, 2] < 0          # the (-1, -1) blob
    if name == "bar":
        assert got[0, 9] == 10


# ---- noise at the percolation densities, one position for every radius 2 ... 127 ----
@pytest.mark.parametrize("group", [name for name, _ in BLS.noise_cases()])
def test_noise_at_every_radius(pt, group):
    cs = dict(BLS.noise_cases())[group]
    first = cs[0]
    h, w = first.frames.shape[1:]
    d_frames = _cuda(np.concatenate([c.frames for c in cs]))       # case k looks at frame k
    bad = []
    with pt.BatchTracker(h, w, 25, (21, 21), True, first.fill) as bt:
        outs = []
        for k, c in enumerate(cs):
            fi = _cuda(np.array([k], np.int32))
            outs.append(bt.blobs(d_frames, _cuda(c.ij), fi, c.radius, 8, c.conns[0], want_sums=True))
        bt.sync()
    nonempty = 0
    for c, (shp, sums) in zip(cs, outs):
        want, words = BLS.reference(c, c.conns[0])
        if not (np.array_equal(sums.cpu().numpy(), words) and _close(shp, want)):
            bad.append((c.radius, sums.cpu().numpy()[0].tolist(), words[0].tolist()))
        nonempty += int(words[0, 0] > 0)
    print(group, "non-empty blobs:", nonempty, "of", len(cs))
    assert not bad, bad[:5]


# ---- narrow frames, clamped positions, min_contrast ----
def test_narrow_frames(pt):
    """9 rows of 1 ... 5 columns: the byte-wise staging path (frames narrower than a dword) and the clamped column at its smallest."""
    rng = np.random.default_rng(3)
    for w in (3, 1, 2, 4, 5):
        wide = np.where(rng.random((2, 9, w + 3)) < 0.4, 40, 128).astype(np.uint8)
        frames = np.ascontiguousarray(wide[:, :, :w])
        ij = np.array([(1, 1), (9, w), (5, (w + 1) // 2), (4, 1), (12, 9)], np.int32)
        fi = np.array([0, 1, 0, 1, 1], np.int32)
        with pt.BatchTracker(9, w, 3, (5, 5), True, 90) as bt:
            for connectivity in (4, 8):
                want, words = BLR.blobs(frames, ij, fi, 3, 90, True, 1, connectivity)
                shp, sums = bt.blobs(_cuda(wide)[:, :, :w], _cuda(ij), _cuda(fi), 3, 1, connectivity, want_sums=True)
                bt.sync()
                assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want), (w, connectivity)


def test_positions_outside_the_frame_and_at_the_corners(pt):
    H, W = BLS.H, BLS.W
    frame = dict(BLS.noise_cases())["overhang 0.42 fill 128"][0].frames[0].copy()
    for ci, cj in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        frame[max(ci - 1, 0):ci + 2, max(cj - 1, 0):cj + 2] = BLS.DARK
    ij = np.array([(1, 1), (1, W), (H, 1), (H, W), (0, 0), (-7, W // 2), (H + 5, W + 9), (H // 2, W + 1), (-200, 500), (1, W // 2), (H, 3)], np.int32)
    fi = np.zeros(len(ij), np.int32)
    for fill in (128, 40):
        with pt.BatchTracker(H, W, 25, (21, 21), True, fill) as bt:
            for R, connectivity in ((5, 4), (12, 8), (25, 4), (40, 8)):
                want, words = BLR.blobs(frame[None], ij, fi, R, fill, True, 8, connectivity)
                shp, sums = bt.blobs(_cuda(frame[None]), _cuda(ij), _cuda(fi), R, 8, connectivity, want_sums=True)
                bt.sync()
                assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want), (fill, R)
                assert np.array_equal(words[0], words[4]) and np.array_equal(words[3], words[6])       # clamped onto the corners
        if fill == 128:
            assert (words[:4, 0] > 0).all()


def test_min_contrast_above_c_gives_zeros_with_b_and_c_kept(pt):
    c = BLS.case("diagonal touch")
    with pt.BatchTracker(BLS.H, BLS.W, 25, (21, 21), True, 128) as bt:
        for mc, n in ((88, 50), (89, 0), (255, 0)):
            shp, sums = bt.blobs(_cuda(c.frames), _cuda(c.ij), None, 12, mc, 8, want_sums=True)
            bt.sync()
            assert sums.cpu().numpy()[0].tolist() == ([50, 125, 125, 725, 625, 725, 128, 88, 50, 0] if n else [0, 0, 0, 0, 0, 0, 128, 88, 0, 0])
            assert bool(np.isnan(shp.cpu().numpy()).all()) == (n == 0)


# ---- shapes of calls ----
def _raw(pt, bt, d_frames, d_ij, d_fi, R, mc, conn, want_sums, want_shape, n=None):
    """pdog_blob itself, with either output NULL; the outputs start at -1."""
    import torch
    n = d_ij.shape[0] if n is None else n
    sums = torch.full((max(n, 1), 10), -1, dtype=torch.int32, device="cuda") if want_sums else None
    shp = torch.full((max(n, 1), 6), -1.0, dtype=torch.float64, device="cuda") if want_shape else None
    bt.use_torch_stream()
    rc = pt.lib().pdog_blob(bt._h, C.c_void_p(d_frames.data_ptr()), d_frames.stride(0), d_frames.stride(1), d_frames.shape[0],
                            C.c_void_p(d_fi.data_ptr()) if d_fi is not None else None, C.c_void_p(d_ij.data_ptr()), n, R, mc, conn,
                            C.c_void_p(sums.data_ptr()) if want_sums else None, C.c_void_p(shp.data_ptr()) if want_shape else None)
    assert rc == 0, pt.lib().pdog_last_error()
    return sums, shp


def test_shapes_of_calls(pt):
    """512 positions at R = 25 on 8 noisy ellipse frames in one call; the frame index given and NULL; either output alone."""
    import torch
    rng = np.random.default_rng(12)
    frames = SS.case("ellipse (12, 5) R 25 dark").frames[:8]
    d_frames = _cuda(frames)
    n = 512
    ij = np.stack([rng.integers(-2, SS.H + 3, n), rng.integers(-2, SS.W + 3, n)], 1).astype(np.int32)
    ij[:384] = np.stack([rng.integers(52, 67, 384), rng.integers(72, 91, 384)], 1)      # on and around the ellipses
    fi = rng.integers(0, 8, n).astype(np.int32)
    d_ij, d_fi = _cuda(ij), _cuda(fi)
    with pt.BatchTracker(SS.H, SS.W, 25, (21, 21), True, 128) as bt:
        for connectivity in (4, 8):
            want, words = BLR.blobs(frames, ij, fi, 25, 128, True, 8, connectivity)
            shp, sums = bt.blobs(d_frames, d_ij, d_fi, None, 8, connectivity, want_sums=True)         # the default radius: 25
            assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want)
            assert (words[:, 0] > 0).sum() > 200 and (words[:, 0] == 0).sum() > 50
        # sums only, floats only: each equal to the pair's
        only_sums, none = _raw(pt, bt, d_frames, d_ij, d_fi, 25, 8, 8, True, False)
        assert none is None and torch.equal(only_sums, sums)
        none, only_shp = _raw(pt, bt, d_frames, d_ij, d_fi, 25, 8, 8, False, True)
        assert none is None and np.array_equal(_bits(only_shp), _bits(shp))
        assert np.array_equal(_bits(bt.blobs(d_frames, d_ij, d_fi, 25, 8)), _bits(shp))              # connectivity 8 is the default
        # without an index: position b on frame b
        a = bt.blobs(d_frames, d_ij[:8], None, 25, 8, 8, want_sums=True)
        b = bt.blobs(d_frames, d_ij[:8], torch.arange(8, dtype=torch.int32, device="cuda"), 25, 8, 8, want_sums=True)
        assert torch.equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        assert np.array_equal(a[1].cpu().numpy(), BLR.blobs(frames, ij[:8], None, 25, 128, True, 8, 8)[1])
        # n = 1 and n = 0
        one = bt.blobs(d_frames, d_ij[7:8], d_fi[7:8], 25, 8, 8, want_sums=True)
        assert torch.equal(one[1], sums[7:8]) and np.array_equal(_bits(one[0]), _bits(shp[7:8]))
        s0, f0 = _raw(pt, bt, d_frames, d_ij, d_fi, 25, 8, 8, True, True, n=0)
        bt.sync()
        assert (s0 == -1).all() and (f0 == -1.0).all()
        out = bt.blobs(d_frames, d_ij[:0], d_fi[:0], 25, 8, 8, want_sums=True)
        assert out[0].shape == (0, 6) and out[1].shape == (0, 10)


def test_tracker_blob_on_its_current_frame(pt):
    c = SS.case("second object R 25")
    t = pt.Tracker(c.frames[0], 25, (21, 21), True)
    ref, rw = BLR.blobs(c.frames, c.ij, None, 25, t.img.fillvalue, True, 8, 4)
    v, s = t.blob(tuple(c.ij[0]), 25, connectivity=4, want_sums=True)
    assert s == tuple(int(x) for x in rw[0]) and s[0] == 113 and s[8] == 142 and _close(np.array(v), ref[0])
    assert t.blob(tuple(c.ij[0])) == v and (v[0], v[1]) == (60.0, 80.0)         # radius ceil(target_width) = 25, connectivity 8
    assert t.shape(tuple(c.ij[0]), want_sums=True)[1][0] == 142                  # the shape rule counts the second object
    t.close()


# ---- frame stacks behind other layouts ----
RH, RW, RNF = 97, 131, 3


def test_layouts_equal_their_contiguous_twin(pt):
    import torch
    rng = np.random.default_rng(77)
    frames = np.where(rng.random((RNF, RH, RW)) < 0.3, 40, 128).astype(np.uint8)
    ij = np.stack([rng.integers(-3, RH + 4, 48), rng.integers(-3, RW + 4, 48)], 1).astype(np.int32)
    fi = rng.integers(0, RNF, 48).astype(np.int32)
    for k, p in enumerate(ij):                    # a dark 3 x 3 under every position
        i, j = min(max(p[0], 1), RH) - 1, min(max(p[1], 1), RW) - 1
        frames[fi[k], max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = 40
    d_ij, d_fi = _cuda(ij), _cuda(fi)
    radii = ((4, 4), (25, 8), (40, 4))             # both tiers
    with pt.BatchTracker(RH, RW, 25, (21, 21), True, 250) as bt:
        twin = {}
        for R, conn in radii:
            twin[R] = bt.blobs(_cuda(frames), d_ij, d_fi, R, 8, conn, want_sums=True)
            words = BLR.blobs(frames, ij, fi, R, 250, True, 8, conn)[1]
            assert np.array_equal(twin[R][1].cpu().numpy(), words) and (words[:, 0] > 0).sum() > 24
        for slack, base, gap in [(1, 32 + 1, 7), (3, 32 + 2, 0), (64, 32 + 13, 7), (0, 32 + 5, 0), (19, 2 * RW + 5, 3 * RW + 7)]:
            for poison in (0, 255, 40):           # the bytes behind a row's frame_w, between the frames and in front of them
                d = LF.to_device(LF.make(frames, slack, base, gap, poison))
                for R, conn in radii:
                    shp, sums = bt.blobs(d, d_ij, d_fi, R, 8, conn, want_sums=True)
                    assert torch.equal(sums, twin[R][1]), (slack, base, gap, poison, R)
                    assert np.array_equal(_bits(shp), _bits(twin[R][0])), (slack, base, gap, poison, R)
        # frames that overlap, and frames that are all the same memory
        tall = np.concatenate([frames[0]] + [frames[k][RH - 64:] for k in range(1, RNF)])
        for lay in (LF.overlapping(tall, RNF, RH, 64, 19, 32 + 7, 5), LF.aliased(frames[0], RNF, 3, 32 + 5, 5)):
            want = bt.blobs(_cuda(lay.twin()), d_ij, d_fi, 25, 8, 8, want_sums=True)
            shp, sums = bt.blobs(LF.to_device(lay), d_ij, d_fi, 25, 8, 8, want_sums=True)
            assert torch.equal(sums, want[1]) and np.array_equal(_bits(shp), _bits(want[0])), lay.describe()
        bt.sync()


# ---- refusals ----
def test_error_returns(pt):
    import torch
    L, E = pt.lib(), pt._lib.PDOG_E_ARG
    h, w = 40, 50
    bt = pt.BatchTracker(h, w, 10, (21, 21), True, 128)
    bt.use_torch_stream()
    f = torch.full((2, h, w), 128, dtype=torch.uint8, device="cuda")
    f[:, 3:8, 3:8] = 0
    ij = torch.tensor([[5, 5], [6, 6]], dtype=torch.int32, device="cuda")
    sums = torch.full((2, 10), -3, dtype=torch.int32, device="cuda")
    shp = torch.full((2, 6), -3.0, dtype=torch.float64, device="cuda")
    fi = torch.zeros(2, dtype=torch.int32, device="cuda")
    P = lambda t_: C.c_void_p(t_.data_ptr())  # noqa: E731

    def call(t=bt._h, frames=P(f), fs=h * w, rs=w, nf=2, index=None, pos=P(ij), n=2, R=5, mc=8, conn=8, osums=P(sums), oshape=P(shp)):
        return L.pdog_blob(t, frames, fs, rs, nf, index, pos, n, R, mc, conn, osums, oshape)

    refused = [dict(conn=0), dict(conn=6), dict(conn=-8), dict(osums=None, oshape=None), dict(R=1), dict(R=128), dict(mc=0), dict(mc=256),
               dict(n=2, nf=1), dict(t=None), dict(frames=None), dict(pos=None), dict(n=-1), dict(nf=0), dict(rs=w - 1),
               dict(rs=(1 << 21) + 1), dict(fs=-1), dict(R=-1), dict(mc=-8), dict(conn=5), dict(conn=1 << 20)]
    for kw in refused:
        assert call(**kw) == E, kw
        msg = L.pdog_last_error()
        assert b"pdog_blob" in msg, kw
        if "conn" in kw:
            assert b"connectivity " + str(kw["conn"]).encode() in msg           # the text names the value
        bt.sync()
        assert (sums == -3).all() and (shp == -3.0).all(), kw                   # nothing was launched
        assert call() == 0, kw                                                  # and a valid call on the same tracker succeeds
        bt.sync()
        assert sums[:, 0].cpu().tolist() == [25, 25] and sums[:, 8].cpu().tolist() == [25, 25]
        sums.fill_(-3)
        shp.fill_(-3.0)
    assert call(n=0) == 0                                   # n == 0 does nothing
    bt.sync()
    assert (sums == -3).all() and (shp == -3.0).all()
    assert call(n=2, nf=1, index=P(fi)) == 0 and call(R=0) == 0 and call(R=2, conn=4) == 0 and call(R=127, mc=255) == 0
    assert call(osums=None) == 0 and call(oshape=None) == 0
    bt.sync()
    bt.close()
    # the binding's checks come before any address reaches the library
    with pt.BatchTracker(h, w, 10, (21, 21), True, 128) as b2:
        for exc, kw in ((ValueError, dict(connectivity=6)), (TypeError, dict(connectivity=8.0)), (ValueError, dict(radius=1)),
                        (ValueError, dict(radius=128)), (ValueError, dict(min_contrast=0)), (TypeError, dict(min_contrast=None))):
            with pytest.raises(exc):
                b2.blobs(f, ij, **kw)
        with pytest.raises(TypeError):
            b2.blobs(f.cpu(), ij)
        with pytest.raises(ValueError):
            b2.blobs(f[:, :, :w - 1], ij)


# ---- the track functions' keyword ----
def _second_object_clip(nf=12):
    """The "second object" scene as a clip: the disc of value 60 drifts to the right, the smaller, darker one keeps 14 px to its
    right."""
    frames = np.full((nf, SS.H, SS.W), 128, np.uint8)
    yy, xx = np.ogrid[0:SS.H, 0:SS.W]
    for k in range(nf):
        frames[k][(yy - 59) ** 2 + (xx - (60 + 2 * k)) ** 2 <= 36] = 60
        frames[k][(yy - 59) ** 2 + (xx - (74 + 2 * k)) ** 2 <= 9] = 0
    return frames


def test_track_video_shape_connectivity(pt):
    import torch
    frames = _second_object_clip()
    nf = len(frames)
    d_frames = _cuda(frames)
    kw = dict(rate=24, start=0, stop=nf / 24, fps=24, target_width=12, window_size=21, darker_target=True, start_locations=[("ij", (60, 61))])
    base = pt.track_video(d_frames, shape=True, shape_radius=25, **kw)
    res = pt.track_video(d_frames, shape=True, shape_radius=25, shape_connectivity=8, **kw)
    none = pt.track_video(d_frames, shape=True, shape_radius=25, shape_connectivity=None, **kw)
    assert len(res) == len(base) == 3 and np.array_equal(res[0], base[0]) and torch.equal(res[1], base[1])
    assert np.array_equal(_bits(none[2]), _bits(base[2]))                      # None is the shape rule, bit for bit
    fi = torch.arange(nf, dtype=torch.int32, device="cuda")
    pos = res[1].reshape(-1, 2).contiguous()
    with pt.BatchTracker(SS.H, SS.W, 12, (21, 21), True, pt.mode(frames[0])) as bt:
        want, sums = bt.blobs(d_frames, pos, fi, 25, 8, 8, want_sums=True)
        four = bt.blobs(d_frames, pos, fi, 25, 8, 4)
        plain = bt.shapes(d_frames, pos, fi, 25, 8)
        bt.sync()
    assert np.array_equal(_bits(res[2]), _bits(want.view(1, nf, 6))) and np.array_equal(_bits(base[2]), _bits(plain.view(1, nf, 6)))
    ref, words = BLR.blobs(frames, pos.cpu().numpy(), None, 25, pt.mode(frames[0]), True, 8, 8)
    assert np.array_equal(sums.cpu().numpy(), words) and _close(res[2].view(-1, 6), ref)
    assert (words[:, 0] < words[:, 8]).all()                                    # two objects in every patch, one measured
    res4 = pt.track_video(d_frames, shape=True, shape_radius=25, shape_connectivity=4, **kw)
    assert np.array_equal(_bits(res4[2]), _bits(four.view(1, nf, 6)))
    with pytest.raises(ValueError, match="shape_connectivity"):
        pt.track_video(d_frames, shape_connectivity=8, **kw)
    with pytest.raises(ValueError, match="shape_connectivity"):
        pt.track_frames(list(frames), shape_connectivity=8)
    with pytest.raises(ValueError, match="shape_connectivity"):
        pt.track_segments([list(frames)], shape_connectivity=4)


def _video_args(sc, **kw):
    return dict(rate=24, start=0, stop=sc.nf / 24, fps=24, target_width=sc.tw, window_size=sc.ws, darker_target=sc.darker,
                start_locations=[("ij", s) for s in sc.starts], **kw)


def test_track_video_blobs_on_the_subtracted_frames(pt):
    import torch
    sc = BS.scene(True, False)
    d_frames = _cuda(sc.frames)
    K = 9
    base = pt.track_video(d_frames, background=K, **_video_args(sc))
    first = None
    for chunk in (1, 7, 60):
        res = pt.track_video(d_frames, background=K, background_chunk=chunk, shape=True, shape_connectivity=8, **_video_args(sc))
        assert len(res) == 3 and np.array_equal(res[0], base[0]) and torch.equal(res[1], base[1])
        first = first or res
        assert np.array_equal(_bits(res[2]), _bits(first[2])), chunk
    sub = BR.subtract(sc.frames, BR.median(sc.frames, BR.samples(range(sc.nf), K)))
    fi = torch.arange(sc.nf, dtype=torch.int32, device="cuda")
    with pt.BatchTracker(*sc.hw, sc.tw, (sc.ws, sc.ws), sc.darker, pt.mode(sub[0])) as bt:
        want = bt.blobs(_cuda(sub), first[1].reshape(-1, 2).contiguous(), fi).view(1, sc.nf, 6)
        bt.sync()
    assert np.array_equal(_bits(first[2]), _bits(want))
    ref, words = BLR.blobs(sub, first[1].reshape(-1, 2).cpu().numpy(), None, 10, pt.mode(sub[0]), True, 8, 8)
    assert _close(first[2].view(-1, 6), ref) and (words[:, 0] > 0).all()


def test_track_frames_and_segments_shape_connectivity(pt):
    frames = list(_second_object_clip())
    kw = dict(target_width=12, start_location=("ij", (60, 61)), darker_target=True, window_size=21)
    plain = pt.track_frames(frames, **kw)
    res = pt.track_frames(frames, shape=True, shape_radius=25, shape_connectivity=8, **kw)
    old = pt.track_frames(frames, shape=True, shape_radius=25, **kw)
    assert len(res) == 2 and res[0] == plain == old[0]
    fill = pt.mode(frames[0])
    ref, words = BLR.blobs(np.stack(frames), np.array(plain, np.int32), None, 25, fill, True, 8, 8)
    assert _close(np.array(res[1]), ref) and (words[:, 0] < words[:, 8]).all()
    assert not _close(np.array(old[1]), ref)                                    # the shape rule measures both objects
    segs = [frames[:5], frames[5:]]
    p2 = pt.track_segments(segs, [kw["start_location"], None], target_width=12, window_size=21)
    r2 = pt.track_segments(segs, [kw["start_location"], None], target_width=12, window_size=21, shape=True, shape_radius=25, shape_connectivity=4)
    assert len(r2) == 2 and r2[0] == p2 and len(r2[1]) == len(frames)
    for k0, k1 in ((0, 5), (5, len(frames))):
        ref, _ = BLR.blobs(np.stack(frames[k0:k1]), np.array(p2[k0:k1], np.int32), None, 25, pt.mode(frames[k0]), True, 8, 4)
        assert _close(np.array(r2[1][k0:k1]), ref), k0
