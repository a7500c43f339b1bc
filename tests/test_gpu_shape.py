"""pdog_shape on the GPU (shape_kernel, BatchTracker.shapes, Tracker.shape, track_video / track_frames(shape=True)): the eight
integer sums bit for bit and the six floats to 1e-9 (the device's atan2 and hypot) against tests/shape_restatement.py, on
every scene of tests/shape_scenes.py and on seeded positions — corners, edges, clamped ones — for every radius at which the
kernel's loops change shape; frame stacks behind other layouts held to their contiguous twins exactly; the shapes of calls;
every refusal; and the track functions' keyword.  The whole file fails on a library without the symbols."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_restatement as BR  # noqa: E402
import background_scenes as BS  # noqa: E402
import layout_frames as LF  # noqa: E402
import shape_restatement as SR  # noqa: E402
import shape_scenes as SS  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert all(hasattr(m.lib(), name) for name in ("pdog_shape", "pdog_shape_derive", "pdog_shape_headings"))
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    """A float64 tensor or array as int64 words on the host: NaN compares as itself."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _close(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.abs(got[ok] - want[ok]).max(initial=0.0) <= TOL


# ---- every scene ----
@pytest.mark.parametrize("name", [c.name for c in SS.cases()])
def test_every_scene_equals_the_restatement(pt, name):
    c = SS.case(name)
    want, words = SS.reference(c)
    with pt.BatchTracker(SS.H, SS.W, c.tw, (21, 21), c.darker, c.fill) as bt:
        shp, sums = bt.shapes(_cuda(c.frames), _cuda(c.ij), _cuda(c.fi), c.radius or None, c.min_contrast, want_sums=True)
        bt.sync()
    assert np.array_equal(sums.cpu().numpy(), words), name
    assert _close(shp, want), (name, np.nanmax(np.abs(shp.cpu().numpy() - want)))
    # the device's floats are the host's to the tolerance, too
    ij = np.stack([np.clip(c.ij[:, 0], 1, SS.H), np.clip(c.ij[:, 1], 1, SS.W)], 1)
    assert _close(shp, pt.shape_derive(sums, ij))


# ---- radii ----
RH, RW, RNF = 97, 131, 3            # the width is no multiple of 4 on purpose
# the issue's radii, both sides of every power of two the bounding box 2R + 1 crosses (the loops' column count), and both sides
# of the radius at which the tile outgrows the default limit on dynamic LDS (R = 110: 49 504 bytes)
RADII = [2, 3, 4, 7, 8, 12, 15, 16, 25, 31, 32, 63, 64, 109, 110, 127]


def _radii_stack(darker):
    """RNF frames on a floor of 100 +- 3 with discs of contrast 5, 20 and 100 — so that min_contrast decides something —, some
    cut by the border; behind rows of RW + 19 bytes whose slack is random."""
    rng = np.random.default_rng(41 + darker)
    wide = rng.integers(0, 256, (RNF, RH, RW + 19)).astype(np.uint8)
    yy, xx = np.ogrid[0:RH, 0:RW]
    for k in range(RNF):
        f = 100 + rng.integers(-3, 4, (RH, RW))
        for (ci, cj, r, con) in [(0, 0, 6, 100), (RH - 1, RW - 1, 9, 20), (48, 65, 7, 100), (20, 100, 4, 5), (70, 30, 12, 20),
                                 (int(rng.integers(0, RH)), int(rng.integers(0, RW)), 5, 100)]:
            f[(yy - ci) ** 2 + (xx - cj) ** 2 <= r * r] = 100 - con if darker else 100 + con
        wide[k, :, :RW] = np.clip(f, 0, 255)
    return wide


def _radii_positions():
    rng = np.random.default_rng(99)
    fixed = [(1, 1), (1, RW), (RH, 1), (RH, RW), (1, RW // 2), (RH, RW // 3), (RH // 2, 1), (RH // 3, RW), (49, 66), (21, 101), (71, 31),
             (0, 0), (-7, RW // 2), (RH + 5, RW + 9), (RH // 2, RW + 1), (-200, 500)]
    rand = [(int(rng.integers(-3, RH + 4)), int(rng.integers(-3, RW + 4))) for _ in range(64 - len(fixed))]
    return np.array(fixed + rand, np.int32), rng.integers(0, RNF, 64).astype(np.int32)


@pytest.fixture(scope="module")
def radii_stacks():
    import torch
    out = {}
    for darker in (True, False):
        wide = _radii_stack(darker)
        out[darker] = (wide[:, :, :RW], torch.from_numpy(wide).cuda()[:, :, :RW])
    return out


@pytest.mark.parametrize("R", RADII)
def test_radii_on_seeded_positions(pt, radii_stacks, R):
    ij, fi = _radii_positions()
    d_ij, d_fi = _cuda(ij), _cuda(fi)
    for darker, fill, contrasts in ((True, 250, (1, 8, 255)), (False, 3, (8,))):     # the fill far from the floor: it decides the median near corners
        frames, d_frames = radii_stacks[darker]
        assert d_frames.stride(1) == RW + 19
        with pt.BatchTracker(RH, RW, 25, (21, 21), darker, fill) as bt:
            for mc in contrasts:
                want, words = SR.shapes(frames, ij, fi, R, fill, darker, mc)
                shp, sums = bt.shapes(d_frames, d_ij, d_fi, R, mc, want_sums=True)
                bt.sync()
                assert np.array_equal(sums.cpu().numpy(), words), (R, darker, mc)
                assert _close(shp, want), (R, darker, mc)
                if mc == 8:
                    assert (words[:, 0] > 0).any() and ((words[:, 0] == 0).any() or R > 64)      # masks and, at the smaller radii, empty ones


def test_default_radius_is_the_target_width(pt, radii_stacks):
    frames, d_frames = radii_stacks[True]
    ij, fi = _radii_positions()
    for tw, R in ((10, 10), (24.2, 25), (1.5, 2), (300, 127)):
        with pt.BatchTracker(RH, RW, tw, (21, 21), True, 128) as bt:
            assert SR.default_radius(tw) == R
            shp, sums = bt.shapes(d_frames, _cuda(ij[:16]), _cuda(fi[:16]), want_sums=True)
            bt.sync()
        want, words = SR.shapes(frames, ij[:16], fi[:16], R, 128, True, 8)
        assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want), tw


# ---- frame stacks behind other layouts ----
def test_layouts_equal_their_contiguous_twin(pt, radii_stacks):
    import torch
    frames = np.ascontiguousarray(radii_stacks[True][0])
    ij, fi = _radii_positions()
    d_ij, d_fi = _cuda(ij), _cuda(fi)
    with pt.BatchTracker(RH, RW, 25, (21, 21), True, 250) as bt:
        twin = {}
        for R in (3, 25, 64):
            twin[R] = bt.shapes(_cuda(frames), d_ij, d_fi, R, 8, want_sums=True)
            # without an index: position b on frame b
            a = bt.shapes(_cuda(frames), d_ij[:RNF], None, R, 8, want_sums=True)
            b = bt.shapes(_cuda(frames), d_ij[:RNF], torch.arange(RNF, dtype=torch.int32, device="cuda"), R, 8, want_sums=True)
            assert torch.equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        layouts = [(1, 32 + 1, 7), (3, 32 + 2, 0), (64, 32 + 13, 7), (0, 32 + 5, 0), (19, 2 * RW + 5, 3 * RW + 7)]
        for slack, base, gap in layouts:
            for poison in (0, 255, 5):            # the bytes behind a row's frame_w, between the frames and in front of them
                lay = LF.make(frames, slack, base, gap, poison)
                d = LF.to_device(lay)
                for R in (3, 25, 64):
                    shp, sums = bt.shapes(d, d_ij, d_fi, R, 8, want_sums=True)
                    assert torch.equal(sums, twin[R][1]), (lay.describe(), poison, R)
                    assert np.array_equal(_bits(shp), _bits(twin[R][0])), (lay.describe(), poison, R)
        # frames that overlap, and frames that are all the same memory
        tall = np.concatenate([frames[0]] + [frames[k][RH - 64:] for k in range(1, RNF)])
        for lay in (LF.overlapping(tall, RNF, RH, 64, 19, 32 + 7, 5), LF.aliased(frames[0], RNF, 3, 32 + 5, 5)):
            want = bt.shapes(_cuda(lay.twin()), d_ij, d_fi, 25, 8, want_sums=True)
            shp, sums = bt.shapes(LF.to_device(lay), d_ij, d_fi, 25, 8, want_sums=True)
            assert torch.equal(sums, want[1]) and np.array_equal(_bits(shp), _bits(want[0])), lay.describe()
        bt.sync()


def test_narrow_frames(pt):
    """Frames narrower than a dword, and just as wide: the byte-wise path and the clamped column at its smallest."""
    rng = np.random.default_rng(3)
    for w in (1, 2, 3, 4, 5):
        wide = rng.integers(0, 256, (2, 9, w + 3)).astype(np.uint8)
        frames = np.ascontiguousarray(wide[:, :, :w])
        ij = np.array([(1, 1), (9, w), (5, (w + 1) // 2), (4, 1), (12, 9)], np.int32)
        fi = np.array([0, 1, 0, 1, 1], np.int32)
        want, words = SR.shapes(frames, ij, fi, 3, 90, True, 1)
        with pt.BatchTracker(9, w, 3, (5, 5), True, 90) as bt:
            shp, sums = bt.shapes(_cuda(wide)[:, :, :w], _cuda(ij), _cuda(fi), 3, 1, want_sums=True)
            bt.sync()
        assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want), w


# ---- shapes of calls ----
def _raw(pt, bt, d_frames, d_ij, d_fi, R, mc, want_sums, want_shape, n=None):
    """pdog_shape itself, with either output NULL; the outputs start at -1."""
    import torch
    n = d_ij.shape[0] if n is None else n
    sums = torch.full((max(n, 1), 8), -1, dtype=torch.int32, device="cuda") if want_sums else None
    shp = torch.full((max(n, 1), 6), -1.0, dtype=torch.float64, device="cuda") if want_shape else None
    bt.use_torch_stream()
    rc = pt.lib().pdog_shape(bt._h, C.c_void_p(d_frames.data_ptr()), d_frames.stride(0), d_frames.stride(1), d_frames.shape[0],
                             C.c_void_p(d_fi.data_ptr()) if d_fi is not None else None, C.c_void_p(d_ij.data_ptr()), n, R, mc,
                             C.c_void_p(sums.data_ptr()) if want_sums else None, C.c_void_p(shp.data_ptr()) if want_shape else None)
    assert rc == 0, pt.lib().pdog_last_error()
    return sums, shp


def test_shapes_of_calls(pt):
    import torch
    rng = np.random.default_rng(12)
    c = SS.case("ellipse (12, 5) R 25 dark")
    frames = c.frames[:8]
    d_frames = _cuda(frames)
    with pt.BatchTracker(SS.H, SS.W, 25, (21, 21), True, 128) as bt:
        # n = 5000 on 8 frames: more workgroups than the device holds at once
        n = 5000
        ij = np.stack([rng.integers(-2, SS.H + 3, n), rng.integers(-2, SS.W + 3, n)], 1).astype(np.int32)
        ij[:2000] = np.stack([rng.integers(45, 75, 2000), rng.integers(65, 97, 2000)], 1)      # on and around the ellipses
        fi = rng.integers(0, 8, n).astype(np.int32)
        want, words = SR.shapes(frames, ij, fi, 12, 128, True, 8)
        d_ij, d_fi = _cuda(ij), _cuda(fi)
        shp, sums = bt.shapes(d_frames, d_ij, d_fi, 12, 8, want_sums=True)
        assert np.array_equal(sums.cpu().numpy(), words) and _close(shp, want)
        assert (words[:, 0] > 0).sum() > 500 and (words[:, 0] == 0).sum() > 500
        # sums only, floats only: each equal to the pair's
        only_sums, none = _raw(pt, bt, d_frames, d_ij, d_fi, 12, 8, True, False)
        assert none is None and torch.equal(only_sums, sums)
        none, only_shp = _raw(pt, bt, d_frames, d_ij, d_fi, 12, 8, False, True)
        assert none is None and np.array_equal(_bits(only_shp), _bits(shp))
        assert np.array_equal(_bits(bt.shapes(d_frames, d_ij, d_fi, 12, 8)), _bits(shp))
        # n = 1
        one = bt.shapes(d_frames, d_ij[7:8], d_fi[7:8], 12, 8, want_sums=True)
        assert torch.equal(one[1], sums[7:8]) and np.array_equal(_bits(one[0]), _bits(shp[7:8]))
        # n = 0 does nothing
        s0, f0 = _raw(pt, bt, d_frames, d_ij, d_fi, 12, 8, True, True, n=0)
        bt.sync()
        assert (s0 == -1).all() and (f0 == -1.0).all()
        assert bt.shapes(d_frames, d_ij[:0], d_fi[:0], 12, 8).shape == (0, 6)


def test_queued_behind_detect_chains_without_a_host_wait(pt):
    """detect_chains then shapes with no synchronisation in between gives what the synchronised sequence gives, and shapes
    leaves what detection reads alone."""
    import torch
    sc = BS.scene(True)
    nc, nf = 4, 15
    d_clips = _cuda(sc.frames).view(nc, nf, *sc.hw)
    starts = torch.tensor([sc.truth[0][c * nf] for c in range(nc)], dtype=torch.int32, device="cuda")
    with pt.BatchTracker(*sc.hw, sc.tw, (sc.ws, sc.ws), True, pt.mode(sc.frames[0])) as bt:
        out_a = bt.detect_chains(d_clips, starts)
        bt.sync()
        a = bt.shapes(d_clips.flatten(0, 1), out_a.view(-1, 2), None, None, 8, want_sums=True)
        bt.sync()
        out_b = bt.detect_chains(d_clips, starts)
        b = bt.shapes(d_clips.flatten(0, 1), out_b.view(-1, 2), None, None, 8, want_sums=True)
        bt.sync()
        assert torch.equal(out_a, out_b) and torch.equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        want, words = SR.shapes(sc.frames, out_a.view(-1, 2).cpu().numpy(), None, 10, pt.mode(sc.frames[0]), True, 8)
        assert np.array_equal(b[1].cpu().numpy(), words) and _close(b[0], want) and (words[:, 0] > 0).all()
        stats, variant = bt.exact_stats(), bt.info().variant
        out_c = bt.detect_chains(d_clips, starts)
        bt.sync()
        assert torch.equal(out_c, out_a) and bt.info().variant == variant and bt.exact_stats()[:2] == stats[:2]


def test_tracker_shape_on_its_current_frame(pt):
    c = SS.case("ellipse (6, 3) R 12 bright")
    want, words = SS.reference(c)
    k = 9                                                  # position 9 looks at frame 3
    t = pt.Tracker(c.frames[c.fi[k]], 12, (21, 21), False)
    ref, rw = SR.shapes(c.frames, c.ij[k:k + 1], c.fi[k:k + 1], 12, t.img.fillvalue, False, 8)
    v, s = t.shape(tuple(c.ij[k]), 12, want_sums=True)
    assert s == tuple(int(x) for x in rw[0]) and _close(np.array(v), ref[0])
    assert t.shape(tuple(c.ij[k])) == v and len(v) == 6         # the default radius is ceil(target_width) = 12
    t.close()


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
    sums = torch.full((2, 8), -3, dtype=torch.int32, device="cuda")
    shp = torch.full((2, 6), -3.0, dtype=torch.float64, device="cuda")
    fi = torch.zeros(2, dtype=torch.int32, device="cuda")
    P = lambda t_: C.c_void_p(t_.data_ptr())  # noqa: E731

    def call(t=bt._h, frames=P(f), fs=h * w, rs=w, nf=2, index=None, pos=P(ij), n=2, R=5, mc=8, osums=P(sums), oshape=P(shp)):
        return L.pdog_shape(t, frames, fs, rs, nf, index, pos, n, R, mc, osums, oshape)

    refused = [dict(t=None), dict(frames=None), dict(pos=None), dict(osums=None, oshape=None), dict(n=-1), dict(nf=0), dict(nf=-3),
               dict(rs=w - 1), dict(rs=(1 << 21) + 1), dict(fs=-1), dict(n=2, nf=1),
               dict(R=1), dict(R=-1), dict(R=128), dict(R=1 << 20), dict(mc=0), dict(mc=256), dict(mc=-8)]
    for kw in refused:
        assert call(**kw) == E, kw
        assert b"pdog_shape" in L.pdog_last_error(), kw
    assert call(n=0) == 0                                   # n == 0 does nothing
    bt.sync()
    assert (sums == -3).all() and (shp == -3.0).all()       # nothing was written by any of them
    assert call() == 0 and call(n=2, nf=1, index=P(fi)) == 0 and call(R=0) == 0 and call(R=2) == 0 and call(R=127, mc=255) == 0
    assert call(osums=None) == 0 and call(oshape=None) == 0
    bt.sync()
    assert (sums[:, 0] >= 0).all()
    bt.close()
    # the binding's checks come before any address reaches the library
    with pt.BatchTracker(h, w, 10, (21, 21), True, 128) as b2:
        for exc, kw in ((ValueError, dict(radius=1)), (ValueError, dict(radius=128)), (TypeError, dict(radius=2.0)),
                        (ValueError, dict(min_contrast=0)), (TypeError, dict(min_contrast=None))):
            with pytest.raises(exc):
                b2.shapes(f, ij, **kw)
        with pytest.raises(TypeError):
            b2.shapes(f.cpu(), ij)
        with pytest.raises(TypeError):
            b2.shapes(f, ij.long())
        with pytest.raises(ValueError):
            b2.shapes(f[:, :, :w - 1], ij)


# ---- the track functions' keyword ----
def _video_args(sc, **kw):
    return dict(rate=24, start=0, stop=sc.nf / 24, fps=24, target_width=sc.tw, window_size=sc.ws, darker_target=sc.darker,
                start_locations=[("ij", s) for s in sc.starts], **kw)


@pytest.mark.parametrize("loop", ["plain", "predict"])
def test_track_video_shape(pt, loop):
    import torch
    sc = BS.scene(True, True)
    d_frames = _cuda(sc.frames)
    kw = {} if loop == "plain" else {"predict": True}
    base = pt.track_video(d_frames, subpixel=True, **_video_args(sc, **kw))
    res = pt.track_video(d_frames, subpixel=True, shape=True, **_video_args(sc, **kw))
    assert len(res) == len(base) + 1 == (4 if loop == "plain" else 5)
    assert np.array_equal(res[0], base[0]) and all(torch.equal(a, b) for a, b in zip(res[1:-1], base[1:]))
    shp = res[-1]
    assert shp.shape == (2, sc.nf, 6) and shp.dtype == torch.float64 and shp.is_cuda
    fi = torch.arange(sc.nf, dtype=torch.int32, device="cuda").repeat(2)
    with pt.BatchTracker(*sc.hw, sc.tw, (sc.ws, sc.ws), sc.darker, pt.mode(sc.frames[0])) as bt:
        want = bt.shapes(d_frames, res[1].reshape(-1, 2).contiguous(), fi).view(2, sc.nf, 6)
        narrow = bt.shapes(d_frames, res[1].reshape(-1, 2).contiguous(), fi, 7, 30).view(2, sc.nf, 6)
        bt.sync()
    assert np.array_equal(_bits(shp), _bits(want))
    ref, _ = SR.shapes(sc.frames, res[1].reshape(-1, 2).cpu().numpy(), fi.cpu().numpy(), 10, pt.mode(sc.frames[0]), True, 8)
    assert _close(shp.view(-1, 6), ref)
    # the keywords reach the call, and without the others the shape is the only addition
    res2 = pt.track_video(d_frames, shape=True, shape_radius=7, shape_min_contrast=30, **_video_args(sc, **kw))
    assert len(res2) == len(base) and np.array_equal(_bits(res2[-1]), _bits(narrow)) and torch.equal(res2[1], base[1])
    # the second animal, far from the hole, is a disc of width 10 wherever it is tracked
    on = ~torch.isnan(shp[1, :, 5])
    assert on.sum() >= sc.nf - 2 and (shp[1, on, 5] - 10.155).abs().max() < 1.0


def test_track_video_shape_on_the_subtracted_frames(pt):
    import torch
    sc = BS.scene(True, False)
    d_frames = _cuda(sc.frames)
    K = 9
    base = pt.track_video(d_frames, background=K, subpixel=True, **_video_args(sc))
    first = None
    for chunk in (1, 7, 60):
        res = pt.track_video(d_frames, background=K, background_chunk=chunk, subpixel=True, shape=True, **_video_args(sc))
        assert len(res) == 4 and np.array_equal(res[0], base[0]) and torch.equal(res[1], base[1]) and torch.equal(res[2], base[2])
        first = first or res
        assert np.array_equal(_bits(res[3]), _bits(first[3])), chunk
    sub = BR.subtract(sc.frames, BR.median(sc.frames, BR.samples(range(sc.nf), K)))
    fi = torch.arange(sc.nf, dtype=torch.int32, device="cuda")
    with pt.BatchTracker(*sc.hw, sc.tw, (sc.ws, sc.ws), sc.darker, pt.mode(sub[0])) as bt:
        want = bt.shapes(_cuda(sub), first[1].reshape(-1, 2).contiguous(), fi).view(1, sc.nf, 6)
        bt.sync()
    assert np.array_equal(_bits(first[3]), _bits(want))
    ref, words = SR.shapes(sub, first[1].reshape(-1, 2).cpu().numpy(), None, 10, pt.mode(sub[0]), True, 8)
    assert _close(first[3].view(-1, 6), ref)
    # on the subtracted frames the hole is gone, and the animal is a disc of width 10 wherever it does not overlap the hole
    # (there the frame and the model are both the hole's 0, and that part of the animal is not seen)
    far = np.abs(first[1][0, :, 1].cpu().numpy() - (BS.HOLE[1] + 1)) > 12
    assert (words[:, 0] > 0).all() and far.sum() >= 40 and np.abs(ref[far, 5] - 10.155).max() < 1.0


def test_track_frames_and_segments_shape(pt):
    c = SS.case("moving ellipse")
    frames = list(c.frames)
    kw = dict(target_width=25, start_location=("ij", tuple(int(v) for v in c.ij[0])), darker_target=True)
    plain = pt.track_frames(frames, **kw)
    ijs, sub = pt.track_frames(frames, subpixel=True, **kw)
    res = pt.track_frames(frames, subpixel=True, shape=True, **kw)
    assert len(res) == 3 and res[0] == ijs == plain and res[1] == sub
    only = pt.track_frames(frames, shape=True, shape_radius=25, shape_min_contrast=8, **kw)
    assert len(only) == 2 and only[0] == plain
    assert np.array_equal(_bits(np.array(only[1])), _bits(np.array(res[2])))
    fill = pt.mode(c.frames[0])
    ref, _ = SR.shapes(c.frames, np.array(plain, np.int32), None, 25, fill, True, 8)
    got = np.array(res[2])
    assert got.shape == (len(frames), 6) and _close(got, ref)
    with pt.BatchTracker(SS.H, SS.W, 25, (21, 21), True, fill) as bt:
        want = bt.shapes(_cuda(c.frames), _cuda(np.array(plain, np.int32)))
        bt.sync()
    assert np.array_equal(_bits(got), _bits(want))
    # the heading follows the motion, is kept through the stop and turns on the reversal
    hd = np.degrees(pt.headings(got, np.array(plain, np.int32)))
    n, s = SS.MOVE_N, SS.STOP_N
    assert np.abs(hd[1:n + 1] - SS.MOVE_DEG).max() <= 2.0 and np.abs(hd[n + 1 + s:] - (SS.MOVE_DEG - 180)).max() <= 2.0
    # segments: every segment's tracker takes its fill from its own first frame
    segs = [frames[:6], frames[6:13], frames[13:]]
    locs = [kw["start_location"], None, None]
    p2 = pt.track_segments(segs, locs, target_width=25)
    r2 = pt.track_segments(segs, locs, target_width=25, shape=True)
    assert len(r2) == 2 and r2[0] == p2 and len(r2[1]) == len(frames)
    for k0, k1 in ((0, 6), (6, 13), (13, len(frames))):
        ref, _ = SR.shapes(c.frames[k0:k1], np.array(p2[k0:k1], np.int32), None, 25, pt.mode(c.frames[k0]), True, 8)
        assert _close(np.array(r2[1][k0:k1]), ref), k0
