"""Many clips, each tracked as the reference tracks it (pdog_clips_*, BatchTracker.clip_modes / track_clips, track_clips):
positions and modes bit-exact against the per-clip oracle flow of tests/clips_restatement.py.
PARITY UNPINNED: the oracle is our restatement, see oracle/dog_oracle.c."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, TW, WS = 64, 80, 10, (21, 21)


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _modes(pt, oracle, frames, frame_index=None, tune=()):
    """clip_modes of a numpy stack [n, h, w] against oracle.mode_u8 frame for frame; returns the tracker's counters."""
    import torch
    bt = pt.BatchTracker(frames.shape[1], frames.shape[2], TW, WS, True, 0)
    for key, value in tune:
        bt.set_clips_tuning(key, value)
    fi = None if frame_index is None else torch.tensor(frame_index, dtype=torch.int32).cuda()
    got = bt.clip_modes(_cuda(frames), fi)
    bt.sync()
    counters = bt.clips_counters()
    bt.close()
    ref = [oracle.mode_u8(frames[k]) for k in (range(len(frames)) if frame_index is None else frame_index)]
    assert got.dtype == torch.int32 and got.is_cuda and got.cpu().tolist() == ref, (frames.shape, tune)
    return counters


def _tie_frame():
    tie = np.zeros((4, 6), np.uint8)           # exact ties between 1, 2 and 3 (the frame of test_gpu_parity's mode test)
    tie[:, 0] = 1; tie[:, 1] = 2; tie[:, 2] = 3; tie[:, 3] = [2, 1, 3, 9]; tie[:, 4] = [3, 2, 1, 9]; tie[:, 5] = 9
    return tie


def test_clip_modes_match_the_oracle_frame_for_frame(pt, oracle):
    import torch
    rng = np.random.default_rng(21)
    # many small frames: one workgroup per frame
    f64 = np.concatenate([rng.integers(0, a, (100, 64, 64), dtype=np.uint8) for a in (2, 4, 256)])
    assert _modes(pt, oracle, f64)[:2] == (1, 0)
    # count ties in most frames, and the engineered tie
    small = rng.integers(0, 4, (40, 7, 5), dtype=np.uint8)
    ties = sum(np.sort(np.bincount(f.ravel(), minlength=4))[-1] == np.sort(np.bincount(f.ravel(), minlength=4))[-2] for f in small)
    assert ties >= 5
    for tune in ((), (("mode_form", 2),)):
        _modes(pt, oracle, small, tune=tune)
        _modes(pt, oracle, _tie_frame()[None], tune=tune)
    # flat frames (the contended bin), one of them with a single other pixel
    flat = np.stack([np.full((64, 64), v, np.uint8) for v in (0, 7, 200, 255, 31)])
    flat[4, 63, 63] = 30
    for tune in ((), (("mode_form", 2),)):
        _modes(pt, oracle, flat, tune=tune)
    # one large frame: several workgroups per frame and the resolving launch
    for alphabet in (4, 256):
        big = rng.integers(100, 100 + alphabet, (1, 1080, 1920)).astype(np.uint8)
        assert _modes(pt, oracle, big)[:2] == (0, 1)
    assert _modes(pt, oracle, big, tune=(("mode_form", 1),))[:2] == (1, 0)
    # rows that are not 16-byte aligned: w = 321, and a column-sliced view
    odd = rng.integers(0, 4, (5, 33, 321), dtype=np.uint8)
    for tune in ((), (("mode_form", 2),)):
        _modes(pt, oracle, odd, tune=tune)
    base = rng.integers(0, 5, (6, 50, 80), dtype=np.uint8)
    view = _cuda(base)[:, :, 10:47]
    bt = pt.BatchTracker(50, 37, TW, WS, True, 0)
    assert not view.is_contiguous() and view.stride(1) == 80
    for form in (0, 2):
        bt.set_clips_tuning("mode_form", form)
        assert bt.clip_modes(view).cpu().tolist() == [oracle.mode_u8(base[k][:, 10:47]) for k in range(6)]
    # nothing to do
    bt.set_clips_tuning("mode_form", 0)
    before = bt.clips_counters()
    empty = bt.clip_modes(view, torch.empty((0,), dtype=torch.int32).cuda())
    assert empty.shape == (0,) and bt.clips_counters() == before
    bt.close()
    # a frame index with repeats and in reverse order
    idx = list(range(19, -1, -1)) + [3, 3, 7, 0, 3]
    _modes(pt, oracle, f64[90:110], frame_index=idx)
    _modes(pt, oracle, f64[90:110], frame_index=idx, tune=(("mode_form", 2),))


# ---- the clips of tests 2, 4 and 5: four backgrounds, discs walking near the borders ----
_CLIPS = {}


def _four_clips(oracle):
    if not _CLIPS:
        rng = np.random.default_rng(7)
        spec = ((200, (6, 7), (1, 1)), (60, (58, 72), (-1, 0)), (128, (5, 40), (0, 2)), (230, (32, 40), (0, 1)))
        clips = [cr.make_clip(H, W, TW, b, s, d, 6, rng) for b, s, d in spec]
        starts = [s for _, s, _ in spec]
        own = [oracle.mode_u8(c[0]) for c in clips]
        _CLIPS.update(clips=clips, starts=starts, own=own,
                      own_chains=[cr.chain(oracle, c, TW, WS, True, s) for c, s in zip(clips, starts)],
                      shared_chains=[cr.chain(oracle, c, TW, WS, True, s, fill=own[0]) for c, s in zip(clips, starts)])
    return _CLIPS


def _as_lists(t):
    return [[tuple(int(v) for v in r) for r in clip] for clip in t.cpu().numpy()]


def test_track_clips_gives_every_clip_its_own_fill(pt, oracle):
    import torch
    d = _four_clips(oracle)
    assert len(set(d["own"])) == 4
    assert any(a != b for a, b in zip(d["own_chains"], d["shared_chains"])), "the recipe must make the fill matter"
    frames = _cuda(np.stack(d["clips"]))
    starts = torch.tensor(d["starts"], dtype=torch.int32).cuda()
    bt = pt.BatchTracker(H, W, TW, WS, True, d["own"][0])
    out = bt.track_clips(frames, starts, fills=d["own"])
    bt.sync()
    assert _as_lists(out) == d["own_chains"]
    assert bt.info().fill == d["own"][0]
    assert bt.clips_counters()[2] == 6 * 4            # a batch per frame and fill group
    shared = bt.detect_chains(frames, starts)          # the difference is the fill and nothing else
    bt.sync()
    assert _as_lists(shared) == d["shared_chains"]
    # fills as a tensor, tracker under another fill: the same positions, and that fill back afterwards
    bt.set_fill(3)
    out = bt.track_clips(frames, starts, fills=torch.tensor(d["own"]).cuda())
    bt.sync()
    assert _as_lists(out) == d["own_chains"] and bt.info().fill == 3
    bt.close()


def test_track_clips_first_one_keeps_the_given_start(pt, oracle):
    import torch
    rng = np.random.default_rng(3)
    clip = cr.make_clip(H, W, TW, 150, (43, 40), (0, 1), 5, rng)
    p = cr.bootstrap(oracle, clip[0], TW, WS, True, None)           # the sz .÷ 4 window's answer
    ot_first = cr.chain(oracle, clip, TW, WS, True, p, first=0)
    assert ot_first[0] != p, "re-detecting frame 0 from the auto-detected position must move it"
    ref1 = cr.chain(oracle, clip, TW, WS, True, p, first=1)
    assert ref1[0] == p
    other = cr.make_clip(H, W, TW, 90, (20, 30), (1, 0), 5, rng)
    q = (21, 28)
    frames = _cuda(np.stack([clip, other]))
    starts = torch.tensor([p, q], dtype=torch.int32).cuda()
    fills = [oracle.mode_u8(clip[0]), oracle.mode_u8(other[0])]
    bt = pt.BatchTracker(H, W, TW, WS, True, 0)
    got1 = _as_lists(bt.track_clips(frames, starts, fills=fills, first=1))
    got0 = _as_lists(bt.track_clips(frames, starts, fills=fills, first=0))
    bt.sync()
    bt.close()
    assert got1 == [ref1, cr.chain(oracle, other, TW, WS, True, q, first=1)]
    assert got0 == [ot_first, cr.chain(oracle, other, TW, WS, True, q, first=0)]
    assert got1[0][0] == p and got0[0] != got1[0]


@pytest.mark.parametrize("first", (0, 1))
def test_track_clips_ragged_lengths_leave_the_rest_untouched(pt, oracle, first):
    import torch
    rng = np.random.default_rng(40 + first)
    lens = [8, 0, 1, 5, 8]
    spec = ((200, (10, 12), (1, 1)), (60, (50, 70), (-1, 0)), (128, (8, 40), (0, 2)), (230, (32, 40), (0, 1)), (60, (60, 20), (-1, 1)))
    clips = [cr.make_clip(H, W, TW, b, s, d, 8, rng) for b, s, d in spec]
    starts = [s for _, s, _ in spec]
    fills = [199, 61, 61, 199, 61]                       # two groups, whatever the clips' own modes are
    refs = [cr.chain(oracle, c, TW, WS, True, s, fill=f, first=first, length=n) for c, s, f, n in zip(clips, starts, fills, lens)]
    frames = _cuda(np.stack(clips))
    bt = pt.BatchTracker(H, W, TW, WS, True, 7)
    out = torch.full((5, 8, 2), -9, dtype=torch.int32).cuda()
    got = bt.track_clips(frames, torch.tensor(starts, dtype=torch.int32).cuda(), fills=fills, lengths=np.array(lens), first=first, out=out)
    bt.sync()
    assert got is out and bt.info().fill == 7
    bt.close()
    got = out.cpu().numpy()
    for c, n in enumerate(lens):
        assert [tuple(int(v) for v in r) for r in got[c, :n]] == refs[c], c
        assert (got[c, n:] == -9).all(), c


def test_track_clips_fast_path_is_detect_chains(pt, oracle):
    import torch
    d = _four_clips(oracle)
    frames = _cuda(np.stack(d["clips"]))
    starts = torch.tensor(d["starts"], dtype=torch.int32).cuda()
    bt = pt.BatchTracker(H, W, TW, WS, True, 5)
    out = bt.track_clips(frames, starts, fills=[d["own"][0]] * 4, lengths=[6] * 4, first=0)
    bt.sync()
    assert bt.clips_counters()[2:] == (0, 1) and bt.info().fill == 5
    bt.set_fill(d["own"][0])
    assert torch.equal(out, bt.detect_chains(frames, starts))
    assert _as_lists(out) == d["shared_chains"]
    out = bt.track_clips(frames, starts)                 # no fills: the tracker's own, the same chain
    bt.sync()
    assert bt.clips_counters()[2:] == (0, 2) and _as_lists(out) == d["shared_chains"]
    bt.close()


def _own_fill_measure(pt, clip, tw, ws, ijs, fill=None):
    """Tracker.measure at every position of one clip, under the clip's own fill (or a forced one)."""
    t = pt.Tracker(clip[0], tw, ws, True)
    if fill is not None:
        pt._lib.check(pt.lib().pdog_set_fill(t._h, int(fill)))
    out = []
    for f, ij in zip(clip, ijs):
        t.img.data[...] = f
        out.append(t.measure(ij))
    t.close()
    return out


def test_top_level_track_clips_is_the_reference_flow_per_clip(pt, oracle):
    import torch
    rng = np.random.default_rng(5)
    sar = 1.25
    spec = ((200, (30, 36), (1, 1)), (60, (57, 71), (-1, 0)), (128, (6, 40), (0, 2)), (200, (32, 40), (0, 1)), (60, (30, 30), (1, 1)), (128, (40, 12), (-1, 1)))
    clips = [cr.make_clip(H, W, TW, b, s, d, 6, rng) for b, s, d in spec]
    locs = [None, ("ij", (56, 70)), (41 * sar, 7.0), None, ("ij", (31, 29)), (14.5 * sar, 38.5)]
    lens = [6, 3, 6, 1, 0, 4]
    refs = [cr.track_clip(oracle, c, TW, WS, True, loc, sar, n) for c, loc, n in zip(clips, locs, lens)]
    frames = _cuda(np.stack(clips))
    out, sub = pt.track_clips(frames, TW, locs, 21, True, sar, lengths=lens, subpixel=True)
    assert out.dtype == torch.int32 and out.shape == (6, 6, 2) and sub.dtype == torch.float64 and sub.shape == (6, 6, 2)
    got, gsub = out.cpu().numpy(), sub.cpu().numpy()
    for c, n in enumerate(lens):
        assert [tuple(int(v) for v in r) for r in got[c, :n]] == refs[c], c
        assert not got[c, n:].any() and not gsub[c, n:].any()
    assert torch.equal(out, pt.track_clips(frames, TW, locs, 21, True, sar, lengths=torch.tensor(lens)))
    # sub-pixel positions: per clip under its own fill, which is not what one fill for all gives near a border
    own = [_own_fill_measure(pt, c, TW, WS, r) for c, r in zip(clips, refs)]
    one = [_own_fill_measure(pt, c, TW, WS, r, fill=oracle.mode_u8(clips[0][0])) for c, r in zip(clips, refs)]
    assert any(a != b for a, b in zip(own, one)), "the recipe must make the fill matter for the sub-pixel positions"
    for c, n in enumerate(lens):
        assert [tuple(r) for r in gsub[c, :n]] == own[c], c
    # a larger window and kernel (l = 65), every clip auto-detected
    tw, ws = 25, (45, 45)
    big = [cr.make_clip(120, 160, tw, b, s, d, 4, rng) for b, s, d in ((90, (50, 70), (2, 3)), (180, (70, 95), (-2, -1)), (90, (64, 84), (1, 1)))]
    out = pt.track_clips(_cuda(np.stack(big)), tw, None, 45)
    assert _as_lists(out) == [cr.track_clip(oracle, c, tw, ws, True, None) for c in big]


def test_top_level_track_clips_raises_for_a_start_outside_the_padded_frame(pt, oracle):
    """Where the reference raises a BoundsError (src/PawsomeTracker.jl:45-46) track_clips raises PdogError, with and without
    subpixel, whether the bad start goes through the tracker proper or sits beside auto-detected clips."""
    d = _four_clips(oracle)
    frames = _cuda(np.stack(d["clips"]))
    far = ("ij", (H + 29 // 2 + 2, 10))          # one row beyond the pad of the l = 29 kernel
    for locs in ([far, ("ij", (58, 72)), ("ij", (5, 40)), ("ij", (32, 40))], [None, far, None, None]):
        for subpixel in (False, True):
            with pytest.raises(pt.PdogError) as e:
                pt.track_clips(frames, TW, locs, 21, subpixel=subpixel)
            assert e.value.code == pt._lib.PDOG_E_RANGE, (locs, subpixel)
    out = pt.track_clips(frames, TW, [("ij", s) for s in d["starts"]], 21)      # and a legal call afterwards is unaffected
    assert _as_lists(out) == d["own_chains"]


def test_clips_argument_errors_launch_nothing(pt, oracle):
    import torch
    L, E = pt.lib(), pt._lib.PDOG_E_ARG
    d = _four_clips(oracle)
    frames = _cuda(np.stack(d["clips"]))
    starts = torch.tensor(d["starts"], dtype=torch.int32).cuda()
    out = torch.full((4, 6, 2), -9, dtype=torch.int32).cuda()
    modes = torch.full((24,), -9, dtype=torch.int32).cuda()
    bt = pt.BatchTracker(H, W, TW, WS, True, 9)
    bt.use_torch_stream()
    h = bt._clips_handle()
    fp, sp, op, mp = (C.c_void_p(t.data_ptr()) for t in (frames, starts, out, modes))
    fs, rs = H * W, W
    keep = []

    def i32(v):
        keep.append(np.ascontiguousarray(v, np.int32))      # (alive until the calls below are over)
        return C.c_void_p(keep[-1].ctypes.data)

    bad_modes = [(None, fp, fs, rs, 24, None, 24, mp), (h, None, fs, rs, 24, None, 24, mp), (h, fp, fs, rs, 24, None, 24, None),
                 (h, fp, fs, rs, 24, None, -1, mp), (h, fp, fs, rs, 0, None, 1, mp), (h, fp, fs, W - 1, 24, None, 24, mp),
                 (h, fp, -1, rs, 24, None, 24, mp), (h, fp, fs, rs, 24, None, 25, mp)]
    for a in bad_modes:
        assert L.pdog_clips_modes(*a) == E, a
    ok_f, ok_l = np.array(d["own"], np.int32), np.full(4, 6, np.int32)
    bad_track = [(None, fp, fs, rs, 6, 4, i32(ok_f), i32(ok_l), 0, sp, op), (h, None, fs, rs, 6, 4, None, None, 0, sp, op),
                 (h, fp, fs, rs, 6, 4, None, None, 0, None, op), (h, fp, fs, rs, 6, 4, None, None, 0, sp, None),
                 (h, fp, fs, rs, 0, 4, None, None, 0, sp, op), (h, fp, fs, rs, 6, 0, None, None, 0, sp, op),
                 (h, fp, fs, W - 1, 6, 4, None, None, 0, sp, op), (h, fp, -1, rs, 6, 4, None, None, 0, sp, op),
                 (h, fp, fs, rs, 6, 4, None, None, 2, sp, op), (h, fp, fs, rs, 6, 4, None, None, -1, sp, op),
                 (h, fp, fs, rs, 6, 4, i32([1, 2, 256, 3]), None, 0, sp, op), (h, fp, fs, rs, 6, 4, i32([1, -1, 2, 3]), None, 0, sp, op),
                 (h, fp, fs, rs, 6, 4, None, i32([6, 7, 6, 6]), 0, sp, op), (h, fp, fs, rs, 6, 4, None, i32([6, -1, 6, 6]), 1, sp, op),
                 (h, fp, fs, rs, 2 ** 30, 4, None, None, 0, sp, op)]     # n_clips * n_frames beyond int32
    for a in bad_track:
        assert L.pdog_clips_track(*a) == E, a
        assert b"pdog_clips" in L.pdog_last_error()
    bt.sync()
    assert bt.clips_counters() == (0, 0, 0, 0) and bt.info().fill == 9
    assert (out == -9).all() and (modes == -9).all() and keep
    # a frame of 2^32 - 1 pixels or more has no 32-bit positions: refused before anything is launched
    huge = pt.BatchTracker(65536, 65536, TW, WS, True, 0)
    huge.use_torch_stream()
    assert L.pdog_clips_modes(huge._clips_handle(), fp, 0, 65536, 1, None, 1, mp) == E
    assert huge.clips_counters() == (0, 0, 0, 0)
    huge.close()
    # a start further outside the frame than the pad: PDOG_E_RANGE from sync(), once, and the tracker stays usable
    hw = bt.info().kernel_len // 2
    far = starts.clone()
    far[2] = torch.tensor([H + hw + 2, 10], dtype=torch.int32)
    bt.track_clips(frames, far, fills=d["own"])
    with pytest.raises(pt.PdogError) as e:
        bt.sync()
    assert e.value.code == pt._lib.PDOG_E_RANGE
    bt.sync()
    got = bt.track_clips(frames, starts, fills=d["own"])
    bt.sync()
    assert _as_lists(got) == d["own_chains"] and bt.info().fill == 9
    bt.close()
