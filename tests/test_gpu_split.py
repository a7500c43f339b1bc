"""pdog_blob_split on the GPU (blob_kernel's split instances in both tiers, BatchTracker.split_blobs, track_video's shape_split):
the twelve integers bit for bit and the six floats to 1e-9 (the device's atan2 and hypot) against tests/split_restatement.py — on
every scene of tests/split_scenes.py, in both layouts, with a frame index and without one, for every radius 2 ... 127 and both
connectivities; one target against pdog_blob; frame stacks behind other layouts held to their contiguous twins exactly; every
refusal; and track_video's keyword under the motion and the exclusive loop, plain and over a subtracted background in chunks.
The whole file fails on a library without the symbol."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_restatement as BR  # noqa: E402
import blob_scenes as BLS  # noqa: E402
import layout_frames as LF  # noqa: E402
import motion_scenes as MS  # noqa: E402
import split_restatement as SPR  # noqa: E402
import split_scenes as SPS  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_blob_split")
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


def _four_ways(bt, d_frames, ij, fi, R, mc, conn):
    """The call set-major and target-major, each with the frame index `fi` ([n_sets, n_targets]) and, where fi is None, without:
    a list of (tag, shape [n_sets, n_targets, 6], sums [n_sets, n_targets, 12]) on the host, target-major ones transposed back."""
    out = []
    for tf in (False, True):
        a = _cuda(ij.transpose(1, 0, 2) if tf else ij)
        f = None if fi is None else _cuda(fi.T if tf else fi)
        shp, sums = bt.split_blobs(d_frames, a, f, R, mc, conn, targets_first=tf, want_sums=True)
        assert shp.shape == a.shape[:2] + (6,) and sums.shape == a.shape[:2] + (12,)
        shp, sums = shp.cpu().numpy(), sums.cpu().numpy()
        out.append(("target-major" if tf else "set-major", shp.transpose(1, 0, 2) if tf else shp, sums.transpose(1, 0, 2) if tf else sums))
    return out


def _run_case(pt, c, connectivity):
    want, words = SPS.reference(c, connectivity)
    h, w = c.frames.shape[1:]
    ns, nt = c.ij.shape[:2]
    index = np.repeat(np.arange(ns, dtype=np.int32)[:, None], nt, 1)
    with pt.BatchTracker(h, w, 25, (21, 21), c.darker, c.fill) as bt:
        d_frames = _cuda(c.frames)
        got = [(tag + ", no index", s, v) for tag, s, v in _four_ways(bt, d_frames, c.ij, None, c.radius, c.min_contrast, connectivity)]
        got += [(tag + ", index", s, v) for tag, s, v in _four_ways(bt, d_frames, c.ij, index, c.radius, c.min_contrast, connectivity)]
        bt.sync()
    print(c.name, connectivity, got[0][2][0].tolist())
    for tag, shp, sums in got:
        bad = (sums != words).any(-1)
        assert not bad.any(), (c.name, connectivity, tag, sums[bad][:4].tolist(), words[bad][:4].tolist())
        assert _close(shp, want), (c.name, connectivity, tag)
    return words


# ---- every scene ----
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", [c.name for c in SPS.cases()])
def test_every_scene_equals_the_restatement(pt, name, connectivity):
    c = SPS.case(name)
    if connectivity not in c.conns:
        connectivity = c.conns[0]
    words = _run_case(pt, c, connectivity)
    if name in SPS.ELLIPSES:
        for k in range(words.shape[1]):
            assert (words[0, k, 11] > 0) == (k in SPS.TOUCHING[name]), (name, k)
    if name == "same pixel":
        assert words[0, 1, 0] == 0 and words[0, 1, 8] > 0 and words[0, 0, 0] > 0
    if name == "rival at 2R":
        assert words[0, 1, 10] == words[0, 1, 8] - 1 and words[0, 1, 11] == 1
    if name == "rival at 2R + 1":
        assert (words[0, :, 10] == words[0, :, 8]).all()


# ---- every radius 2 ... 127: every word boundary of the row, the tier boundary, the dynamic LDS beyond 48 KiB ----
@pytest.mark.parametrize("connectivity", [4, 8])
def test_every_radius(pt, connectivity):
    cs = SPS.radius_cases(connectivity)
    d_frames = _cuda(cs[0].frames)
    with pt.BatchTracker(BLS.BIG, BLS.BIG, 25, (21, 21), True, 128) as bt:
        outs = [bt.split_blobs(d_frames, _cuda(c.ij), None, c.radius, 8, connectivity, want_sums=True) for c in cs]
        outs_t = [bt.split_blobs(d_frames, _cuda(c.ij.transpose(1, 0, 2)), None, c.radius, 8, connectivity, targets_first=True, want_sums=True)
                  for c in cs[::7]]
        bt.sync()
    bad, nonempty, contact = [], 0, 0
    for c, (shp, sums) in zip(cs, outs):
        want, words = SPS.reference(c, connectivity)
        if not (np.array_equal(sums.cpu().numpy(), words) and _close(shp, want)):
            bad.append((c.radius, sums.cpu().numpy()[0].tolist(), words[0].tolist()))
        nonempty += int((words[0, :, 0] > 0).sum())
        contact += int((words[0, :, 11] > 0).sum())
    for c, (shp, sums) in zip(cs[::7], outs_t):
        want, words = SPS.reference(c, connectivity)
        if not (np.array_equal(sums.cpu().numpy().transpose(1, 0, 2), words) and _close(shp.cpu().numpy().transpose(1, 0, 2), want)):
            bad.append((c.radius, "target-major"))
    print("connectivity", connectivity, "non-empty blobs:", nonempty, "with contact:", contact, "of", 3 * len(cs))
    assert not bad, bad[:3]
    assert nonempty > 150 and contact > (60 if connectivity == 8 else 5)       # (at 0.47 under connectivity 4 the blobs stay small)


# ---- several sets, a frame index of its own per position, both layouts, both tiers ----
def test_sets_with_their_own_frame_index(pt):
    rng = np.random.default_rng(5)
    frames = np.where(rng.random((3, 97, 131)) < 0.3, 40, 128).astype(np.uint8)
    ns, nt = 7, 5
    centre = np.stack([rng.integers(-3, 101, ns), rng.integers(-3, 135, ns)], 1)
    ij = (centre[:, None, :] + rng.integers(-9, 10, (ns, nt, 2))).astype(np.int32)
    fi = rng.integers(0, 3, (ns, nt)).astype(np.int32)                 # a rival's frame plays no part: only its position does
    with pt.BatchTracker(97, 131, 25, (21, 21), True, 250) as bt:
        for R, conn in ((3, 8), (12, 4), (31, 8), (40, 4)):
            want, words = SPR.split_blobs(frames, ij, fi, R, 250, True, 8, conn)
            for tag, shp, sums in _four_ways(bt, _cuda(frames), ij, fi, R, 8, conn):
                assert np.array_equal(sums, words) and _close(shp, want), (R, conn, tag)
            assert (words[..., 0] > 0).sum() > 10 and (words[..., 10] < words[..., 8]).sum() > 10
        bt.sync()


# ---- one target per set: pdog_blob's ten integers ----
def test_one_target_equals_pdog_blob(pt):
    import torch
    for c in BLS.cases():
        h, w = c.frames.shape[1:]
        with pt.BatchTracker(h, w, c.tw, (21, 21), c.darker, c.fill) as bt:
            d_frames, d_ij, d_fi = _cuda(c.frames), _cuda(c.ij), _cuda(c.fi)
            for conn in c.conns:
                shp, sums = bt.blobs(d_frames, d_ij, d_fi, c.radius, c.min_contrast, conn, want_sums=True)
                for tf in (False, True):
                    a = d_ij.view(1, -1, 2) if tf else d_ij.view(-1, 1, 2)
                    f = d_fi.view(1, -1) if tf else d_fi.view(-1, 1)
                    s2, w2 = bt.split_blobs(d_frames, a, f, c.radius, c.min_contrast, conn, targets_first=tf, want_sums=True)
                    w2 = w2.view(-1, 12)
                    assert torch.equal(w2[:, :10], sums) and torch.equal(w2[:, 10], sums[:, 8]) and (w2[:, 11] == 0).all(), (c.name, conn, tf)
                    assert np.array_equal(_bits(s2.view(-1, 6)), _bits(shp)), (c.name, conn, tf)
                assert np.array_equal(sums.cpu().numpy(), BLS.reference(c, conn)[1])
            bt.sync()


# ---- frame stacks behind other layouts ----
RH, RW, RNF = 97, 131, 3


def test_layouts_equal_their_contiguous_twin(pt):
    import torch
    rng = np.random.default_rng(78)
    frames = np.where(rng.random((RNF, RH, RW)) < 0.3, 40, 128).astype(np.uint8)
    ns, nt = 12, 4
    centre = np.stack([rng.integers(-3, RH + 4, ns), rng.integers(-3, RW + 4, ns)], 1)
    ij = (centre[:, None, :] + rng.integers(-8, 9, (ns, nt, 2))).astype(np.int32)
    fi = np.repeat(rng.integers(0, RNF, ns).astype(np.int32)[:, None], nt, 1)
    d_ij, d_fi = _cuda(ij), _cuda(fi)
    radii = ((4, 4), (25, 8), (40, 4))             # both tiers
    with pt.BatchTracker(RH, RW, 25, (21, 21), True, 250) as bt:
        twin = {}
        for R, conn in radii:
            twin[R] = bt.split_blobs(_cuda(frames), d_ij, d_fi, R, 8, conn, want_sums=True)
            words = SPR.split_blobs(frames, ij, fi, R, 250, True, 8, conn)[1]
            assert np.array_equal(twin[R][1].cpu().numpy(), words) and (words[..., 0] > 0).sum() > 12
        for slack, base, gap in [(1, 32 + 1, 7), (3, 32 + 2, 0), (64, 32 + 13, 7), (0, 32 + 5, 0), (19, 2 * RW + 5, 3 * RW + 7)]:
            for poison in (0, 255, 40):           # the bytes behind a row's frame_w, between the frames and in front of them
                d = LF.to_device(LF.make(frames, slack, base, gap, poison))
                for R, conn in radii:
                    shp, sums = bt.split_blobs(d, d_ij, d_fi, R, 8, conn, want_sums=True)
                    assert torch.equal(sums, twin[R][1]), (slack, base, gap, poison, R)
                    assert np.array_equal(_bits(shp), _bits(twin[R][0])), (slack, base, gap, poison, R)
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
    ij = torch.tensor([[[5, 5], [30, 40], [6, 6]], [[6, 6], [30, 40], [31, 41]]], dtype=torch.int32, device="cuda")     # [2 sets, 3 targets]
    sums = torch.full((6, 12), -3, dtype=torch.int32, device="cuda")
    shp = torch.full((6, 6), -3.0, dtype=torch.float64, device="cuda")
    fi = torch.zeros(6, dtype=torch.int32, device="cuda")
    P = lambda t_: C.c_void_p(t_.data_ptr())  # noqa: E731
    want = SPR.split_blobs(f.cpu().numpy(), ij.cpu().numpy(), None, 5, 128, True, 8, 8)[1].reshape(6, 12)
    assert want[0, 0] > 0 and want[0, 8] == 25 and want[1, 8] == 0

    def call(t=bt._h, frames=P(f), fs=h * w, rs=w, nf=2, index=None, pos=P(ij), ns=2, nt=3, ss=3, ts=1, R=5, mc=8, conn=8, osums=P(sums),
             oshape=P(shp)):
        return L.pdog_blob_split(t, frames, fs, rs, nf, index, pos, ns, nt, ss, ts, R, mc, conn, osums, oshape)

    refused = [dict(conn=0), dict(conn=6), dict(conn=-8), dict(osums=None, oshape=None), dict(R=1), dict(R=128), dict(mc=0), dict(mc=256),
               dict(nf=1), dict(t=None), dict(frames=None), dict(pos=None), dict(ns=-1), dict(nf=0), dict(rs=w - 1),
               dict(rs=(1 << 21) + 1), dict(fs=-1), dict(R=-1), dict(mc=-8),
               dict(nt=0, ss=0), dict(nt=33, ss=33), dict(nt=-1, ss=-1), dict(ss=4), dict(ss=3, ts=2), dict(ss=1, ts=3), dict(ss=2, ts=1),
               dict(ss=0, ts=0), dict(ss=1, ts=1), dict(ss=6, ts=2)]
    for kw in refused:
        assert call(**kw) == E, kw
        msg = L.pdog_last_error()
        assert b"pdog_blob_split" in msg, kw
        if "conn" in kw:
            assert b"connectivity " + str(kw["conn"]).encode() in msg           # the text names the value
        if "nt" in kw:
            assert b"n_targets " + str(kw["nt"]).encode() in msg
        elif "ss" in kw:
            assert f"({kw['ss']}, {kw.get('ts', 1)})".encode() in msg
        if kw == dict(nf=1):
            assert b"n_sets 2" in msg
        bt.sync()
        assert (sums == -3).all() and (shp == -3.0).all(), kw                   # nothing was launched
        assert call() == 0, kw                                                  # and a valid call on the same tracker succeeds
        bt.sync()
        assert np.array_equal(sums.cpu().numpy(), want), kw
        sums.fill_(-3)
        shp.fill_(-3.0)
    assert call(ns=0) == 0 and call(ns=0, ss=1, ts=0) == 0     # n_sets == 0 does nothing
    bt.sync()
    assert (sums == -3).all() and (shp == -3.0).all()
    assert call(nf=1, index=P(fi)) == 0 and call(R=0) == 0 and call(R=2, conn=4) == 0 and call(R=127, mc=255) == 0
    assert call(osums=None) == 0 and call(oshape=None) == 0
    assert call(ss=1, ts=2) == 0                               # the same memory read target-major: [3 targets, 2 sets]
    assert call(ns=1, nt=6, ss=6, ts=1, nf=1) == 0 and call(ns=6, nt=1, ss=1, ts=1, index=P(fi)) == 0 and call(ns=1, nt=6, ss=1, ts=1) == 0
    bt.sync()
    bt.close()
    # the binding's checks come before any address reaches the library
    with pt.BatchTracker(h, w, 10, (21, 21), True, 128) as b2:
        many = torch.ones((1, 33, 2), dtype=torch.int32, device="cuda")
        for exc, a, kw in ((ValueError, (f, ij), dict(connectivity=6)), (TypeError, (f, ij), dict(connectivity=8.0)), (ValueError, (f, ij), dict(radius=1)),
                           (ValueError, (f, ij), dict(radius=128)), (ValueError, (f, ij), dict(min_contrast=0)), (TypeError, (f, ij), dict(min_contrast=None)),
                           (TypeError, (f, ij), dict(targets_first=None)), (TypeError, (f.cpu(), ij), {}), (ValueError, (f[:, :, :w - 1], ij), {}),
                           (TypeError, (f, ij.view(-1, 2)), {}), (TypeError, (f, ij.long()), {}), (TypeError, (f, ij.cpu()), {}),
                           (ValueError, (f, ij[:, :, :1]), {}), (ValueError, (f, ij.transpose(0, 1)), {}), (ValueError, (f, many), {}),
                           (ValueError, (f, many.transpose(0, 1).contiguous()), dict(targets_first=True)), (ValueError, (f, ij[:, :0]), {}),
                           (TypeError, (f, ij), dict(frame_index=fi)), (TypeError, (f, ij), dict(frame_index=fi.view(2, 3).long())),
                           (ValueError, (f, ij), dict(frame_index=fi.view(3, 2))), (ValueError, (f[:1], ij), {}),
                           (ValueError, (f, ij), dict(targets_first=True))):          # 3 sets on 2 frames and no index
            with pytest.raises(exc) as e:
                b2.split_blobs(*a, **kw)
            assert type(e.value) is exc, kw
        out = b2.split_blobs(f, ij[:0], want_sums=True)
        assert out[0].shape == (0, 3, 6) and out[1].shape == (0, 3, 12)
        assert b2.split_blobs(f, ij, fi.view(2, 3)).shape == (2, 3, 6)


# ---- track_video's keyword ----
def _video_args(sc, **kw):
    return dict(rate=24, start=0, stop=sc.nf / 24, fps=24, target_width=sc.tw, window_size=sc.ws, darker_target=True,
                start_locations=[("ij", s) for s in sc.starts], **kw)


def _flow(frames, out, fill, R):
    """The restatement over a result's positions out [n_targets, m, 2] (host): (shape [n_targets, m, 6], contact [n_targets, m])."""
    shp, words = SPR.split_blobs(frames, out.transpose(1, 0, 2), None, R, fill, True, 8, 8)
    return shp.transpose(1, 0, 2), words[:, :, 11].T


@pytest.mark.parametrize("loop", ["motion", "exclusive"])
def test_track_video_shape_split(pt, loop):
    import torch
    sc = MS.scene("through")
    d_frames = _cuda(sc.frames)
    R = 10                                       # ceil(target_width)
    kw = _video_args(sc, **{loop: True})
    today = pt.track_video(d_frames, shape=True, shape_connectivity=8, **kw)
    off = pt.track_video(d_frames, shape=True, shape_connectivity=8, shape_split=False, **kw)
    assert len(today) == len(off) == 4 and np.array_equal(today[0], off[0])
    assert all(torch.equal(a, b) for a, b in zip(today[1:3], off[1:3])) and np.array_equal(_bits(today[3]), _bits(off[3]))
    res = pt.track_video(d_frames, shape=True, shape_connectivity=8, shape_split=True, **kw)
    assert len(res) == 5 and np.array_equal(res[0], today[0]) and torch.equal(res[1], today[1]) and torch.equal(res[2], today[2])
    shp, contact = res[3], res[4]
    assert shp.shape == (2, sc.nf, 6) and contact.shape == (2, sc.nf) and contact.dtype == torch.int32 and contact.is_contiguous()
    want, touch = _flow(sc.frames, res[1].cpu().numpy(), pt.mode(sc.frames[0]), R)
    assert _close(shp, want)
    assert np.array_equal(contact.cpu().numpy(), touch)
    print(loop, "steps with contact:", np.nonzero((touch > 0).any(0))[0].tolist())
    assert (touch > 0).any() and (touch[:, :8] == 0).all() and (touch[:, -8:] == 0).all()       # they touch in the middle of the clip only
    # where the two are more than 2R apart the split measurement is the blob rule's, bit for bit
    pos = res[1].cpu().numpy().astype(np.int64)
    far = ((pos[0] - pos[1]) ** 2).sum(-1) > (2 * R) ** 2
    assert far.sum() > 10 and np.array_equal(_bits(shp)[:, far], _bits(today[3])[:, far])
    # over a subtracted background, in chunks: one answer
    K = 9
    first = None
    for chunk in (1, 7, 60):
        r = pt.track_video(d_frames, background=K, background_chunk=chunk, shape=True, shape_connectivity=8, shape_split=True, **kw)
        assert len(r) == 5
        first = first or r
        assert torch.equal(r[1], first[1]) and torch.equal(r[4], first[4]) and np.array_equal(_bits(r[3]), _bits(first[3])), chunk
    sub = BR.subtract(sc.frames, BR.median(sc.frames, BR.samples(range(sc.nf), K)))
    want, touch = _flow(sub, first[1].cpu().numpy(), pt.mode(sub[0]), R)
    assert _close(first[3], want) and np.array_equal(first[4].cpu().numpy(), touch)


def test_track_video_shape_split_plain_and_predict(pt):
    import torch
    sc = MS.scene("through")
    d_frames = _cuda(sc.frames)
    for extra in ({}, dict(predict=True)):
        kw = _video_args(sc, **extra)
        today = pt.track_video(d_frames, subpixel=True, shape=True, shape_connectivity=4, **kw)
        res = pt.track_video(d_frames, subpixel=True, shape=True, shape_connectivity=4, shape_split=True, **kw)
        assert len(res) == len(today) + 1 and all(torch.equal(a, b) for a, b in zip(today[1:-1], res[1:-2]))
        shp, words = SPR.split_blobs(sc.frames, res[1].cpu().numpy().transpose(1, 0, 2), None, 10, pt.mode(sc.frames[0]), True, 8, 4)
        assert _close(res[-2], shp.transpose(1, 0, 2)) and np.array_equal(res[-1].cpu().numpy(), words[:, :, 11].T)
    with pytest.raises(ValueError, match="shape_split"):
        pt.track_video(d_frames, shape=True, shape_split=True, **_video_args(sc))
