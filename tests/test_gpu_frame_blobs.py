"""Every connected blob of a whole frame on the GPU (include/pawsome_frame_blobs.h).  Every comparison is exact.

Counts and all twelve words are held bit for bit to tests/frame_blobs_restatement.py (scipy.ndimage.label and integer sums) on
the scenes of tests/frame_blobs_scenes.py — empty and full masks, corner pixels, a spiral, a comb, a checkerboard (whose list
is cut at the cap), staircases through the tile corners, a lattice over every tile border, bars one pixel apart across borders,
noise either side of the percolation thresholds — at both connectivities and both signs, over all frame sizes of
{1, 2, 31, 33, 70} x {1, 63, 64, 65, 127, 129, 200} (tiles are 64 x 64) with more steps than the handle holds in flight, and at
270 x 480 through a table that names a frame twice; the area filter and the cap from both ends; strided, offset, poisoned,
overlapping and aliased stacks of tests/layout_frames.py against their contiguous twins; every refusal, with nothing written;
and track_video(n_targets=3, find="frame") on the bootstrap video, with and without `background`.  The whole file fails on a
library without the symbols.

THE LARGE SHAPES (frame_blobs_scenes.LARGE, the smallest that reach each path): 520 x 520 and 1037 x 1041, where the scan of
the blocks' counts takes two and five passes of 1024 blocks; 3 x 2^21 and 3 024 617 x 1, the widest and the tallest size the
handle admits, whose full frames' Sxx and Syy stand within a millionth of 2^63; 9000 x 64, a single column of 141 tiles.  On
them the words are held to the restatement AND, on the full mask, to the closed forms in Python integers, so that a sum that
wrapped on both sides alike could not pass; every shape must produce a word above 2^32.  Kept blobs are ranked across all scan
passes with a cap above the count (every row compared) and with a cap that cuts the list inside the first pass.  The largest
round a handle takes, 1024 steps in flight, and 1023; a host table overwritten straight after the call returns; outputs one
element into sentinel-filled tensors; the edges of the admitted sizes on the device.
NOT REACHED HERE: a single addend to Syx beyond 2^32 needs y * c > 6.7e7 inside one frame, a frame of more than 6.7e7 pixels,
and frames near 2^30 pixels are out for the same reason — neither runs in seconds."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_blobs_restatement as FR  # noqa: E402
import frame_blobs_scenes as FS  # noqa: E402
import layout_frames as LF  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_frame_blobs") and hasattr(m, "FrameBlobs")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    count, words = (v.cpu().numpy() for v in got)
    assert count.dtype == np.int32 and words.dtype == np.int64
    assert np.array_equal(count, want[0]), (what, count.tolist(), want[0].tolist())
    bad = np.argwhere(words != want[1])
    assert len(bad) == 0, (what, bad[:5].tolist(), words[tuple(bad[0])], want[1][tuple(bad[0])])


# ---- the scenes at every shape ----
@pytest.mark.parametrize("w", FS.WIDTHS)
@pytest.mark.parametrize("h", FS.HEIGHTS)
def test_scenes_equal_the_restatement(pt, h, w):
    n, first = len(FS.NAMES), {}
    with pt.FrameBlobs(h, w, steps_in_flight=4) as fb:                 # 11 scenes: three rounds, the last one short
        for darker in (True, False):
            stack = FS.frames(h, w, darker)
            d = _cuda(stack)
            for conn in (4, 8):
                kw = dict(level=FS.LEVEL[darker], min_contrast=8, connectivity=conn)
                want = FR.find(stack, darker=darker, cap=64, **kw)
                _same(fb.find(d, darker_target=darker, cap=64, **kw), want, (h, w, darker, conn))
                if darker:                                             # both signs see the same blobs
                    first[conn] = want
                else:
                    assert np.array_equal(want[0], first[conn][0]) and np.array_equal(want[1], first[conn][1])
                if min(h, w) >= 2 and h * w >= 130:                    # the checkerboard's list is cut at connectivity 4 only
                    k = FS.NAMES.index("checkerboard")
                    assert want[0][k, 0] == ((h * w + 1) // 2 if conn == 4 else 1) and (conn == 8 or want[0][k, 0] > 64)
    assert n == 11


def test_larger_frame_through_a_table_that_repeats(pt):
    h, w = 270, 480
    names = ("spiral", "noise 0.41", "lattice", "noise 0.59", "staircases")
    stack = np.stack([FS.draw(FS.pattern(name, h, w), True, k) for k, name in enumerate(names)])
    table = [4, 1, 0, 1, 3, 2]
    with pt.FrameBlobs(h, w, steps_in_flight=4) as fb:
        for conn in (4, 8):
            want = FR.find(stack, table, connectivity=conn, cap=100)
            _same(fb.find(_cuda(stack), table, connectivity=conn, cap=100), want, conn)
            assert np.array_equal(want[1][1], want[1][3]) and want[0][2, 0] == 1 and want[1][2, 0, 0] > h * w // 2 - 2 * (h + w)
    # a tensor table, and None: every frame in turn
    import torch
    with pt.FrameBlobs(h, w) as fb:
        _same(fb.find(_cuda(stack), torch.tensor([2, 2])), FR.find(stack, [2, 2]), "tensor table")
        _same(fb.find(_cuda(stack)), FR.find(stack), "no table")
        count, words = fb.find(_cuda(stack), [])
        assert tuple(count.shape) == (0, 2) and tuple(words.shape) == (0, 64, 12)


# ---- the area filter and the cap ----
def test_area_filter_and_cap_cut_the_list_from_both_ends(pt):
    h, w = 70, 200
    stack = FS.frames(h, w)
    d = _cuda(stack)
    k = FS.NAMES.index("noise 0.41")
    sizes = FR.all_blobs(stack[k], connectivity=4)[0][:, 0]
    assert sizes.min() == 1 and sizes.max() > 40
    with pt.FrameBlobs(h, w, steps_in_flight=len(stack)) as fb:
        for lo, hi in ((1, None), (2, None), (1, 1), (3, 9), (10, 40), (int(sizes.max()), int(sizes.max())), (h * w, None)):
            n_kept = int(((sizes >= lo) & (sizes <= (hi or h * w))).sum())
            for cap in sorted({1, 2, 64, max(n_kept, 1), n_kept + 3}):        # cap = 1, cap = the count, room to spare
                kw = dict(connectivity=4, min_area=lo, max_area=hi, cap=cap)
                want = FR.find(stack, **kw)
                assert want[0][k, 0] == n_kept
                _same(fb.find(d, **kw), want, (lo, hi, cap))
                assert not want[1][k, min(n_kept, cap):].any()                  # rows behind the count are zero
    # other levels and contrasts: the mask is the rule's, at the ends of both ranges
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (3, 33, 65), dtype=np.uint8)
    with pt.FrameBlobs(33, 65) as fb:
        for level, mc, darker in ((0, 1, False), (255, 1, True), (255, 255, True), (0, 255, False), (0, 1, True), (77, 30, True), (200, 3, False)):
            kw = dict(level=level, min_contrast=mc, connectivity=8, cap=40)
            _same(fb.find(_cuda(noise), darker_target=darker, **kw), FR.find(noise, darker=darker, **kw), (level, mc, darker))


# ---- layouts ----
def test_strided_offset_and_poisoned_stacks_equal_their_twins(pt):
    h, w = 70, 129
    names = ("noise 0.41", "lattice", "corners", "full")
    for darker in (True, False):
        poison = LF.poison_for(darker)                                  # slack read as pixels would join the mask
        stack = np.stack([FS.draw(FS.pattern(name, h, w), darker, k) for k, name in enumerate(names)])
        kw = dict(level=FS.LEVEL[darker], connectivity=8, cap=50)
        want = FR.find(stack, [3, 0, 1, 2, 0], darker=darker, **kw)
        with pt.FrameBlobs(h, w, steps_in_flight=2) as fb:
            for slack, base, gap in ((0, 0, 0), (1, 33, 7), (3, 34, 0), (19, 2 * w + 5, 3 * w + 7), (64, 45, 7), (0, 1, 1), (127, 3, 0)):
                lay = LF.make(stack, slack, base, gap, poison)
                d = LF.to_device(lay)
                assert np.array_equal(lay.twin(), stack)
                _same(fb.find(d, [3, 0, 1, 2, 0], darker_target=darker, **kw), want, lay.describe())
            # frames that overlap (rows of one tall image) and frames that are all the same memory
            tall = np.concatenate([stack[0], stack[1][h - 40:], stack[2][h - 40:]])
            for lay in (LF.overlapping(tall, 3, h, 40, 19, 39, poison), LF.aliased(stack[0], 3, 3, 37, poison)):
                _same(fb.find(LF.to_device(lay), darker_target=darker, **kw), FR.find(lay.twin(), darker=darker, **kw), lay.describe())


# ---- refusals ----
def test_every_refusal_names_its_value_and_writes_nothing(pt):
    import torch
    from pawsometracker_jl_amd import _lib
    h, w, nf, cap = 33, 65, 3, 4
    frames = _cuda(FS.frames(h, w)[:nf])
    words = torch.full((2, cap, 12), SENTINEL, dtype=torch.int64, device="cuda")
    count = torch.full((2, 2), SENTINEL, dtype=torch.int32, device="cuda")
    table = np.array([0, 2], np.int32)
    L = pt.lib()
    with pt.FrameBlobs(h, w) as fb:
        ok = dict(fb=fb._h, stream=None, frames=C.c_void_p(frames.data_ptr()), fs=h * w, rs=w, nf=nf, table=C.c_void_p(table.ctypes.data), ns=2,
                  level=128, darker=1, mc=8, conn=8, lo=1, hi=h * w, cap=cap, words=C.c_void_p(words.data_ptr()), count=C.c_void_p(count.data_ptr()))
        bad_table = np.array([0, 3], np.int32)
        neg_table = np.array([-1, 0], np.int32)
        cases = [(dict(fb=None), "null handle"), (dict(frames=None), "null pointer (d_frames)"), (dict(table=None), "null pointer (h_table)"),
                 (dict(words=None), "null pointer (d_out_words)"), (dict(count=None), "null pointer (d_out_count)"),
                 (dict(table=C.c_void_p(bad_table.ctypes.data)), "table entry 1 is 3"), (dict(table=C.c_void_p(neg_table.ctypes.data)), "table entry 0 is -1"),
                 (dict(level=-1), "level -1"), (dict(level=256), "level 256"), (dict(mc=0), "min_contrast 0"), (dict(mc=256), "min_contrast 256"),
                 (dict(conn=6), "connectivity 6"), (dict(conn=0), "connectivity 0"), (dict(lo=0), "min_area 0"), (dict(lo=5, hi=4), "max_area 4"),
                 (dict(cap=0), "cap 0"), (dict(rs=w - 1), f"row_stride {w - 1}"), (dict(rs=_lib.PDOG_MAX_ROW_STRIDE + 1), "row_stride"),
                 (dict(fs=-1), "frame_stride -1"), (dict(nf=0), "n_frames 0"), (dict(ns=-1), "n_steps -1")]
        for change, text in cases:
            a = {**ok, **change}
            assert L.pdog_frame_blobs(*a.values()) == _lib.PDOG_E_ARG, change
            msg = L.pdog_last_error().decode()
            assert msg.startswith("pdog_frame_blobs: ") and text in msg, (change, msg)
        torch.cuda.synchronize()
        assert bool((words == SENTINEL).all()) and bool((count == SENTINEL).all())           # nothing was written
        # n_steps == 0 does nothing, whatever the pointers
        assert L.pdog_frame_blobs(*{**ok, "ns": 0, "table": None, "words": None, "count": None}.values()) == _lib.PDOG_OK
        torch.cuda.synchronize()
        assert bool((words == SENTINEL).all()) and bool((count == SENTINEL).all())
        # and the call as it stands works, on another stream than the last too
        assert L.pdog_frame_blobs(*ok.values()) == _lib.PDOG_OK
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again = fb.find(frames, table, cap=cap)
        side.synchronize()
        _same((count, words), FR.find(frames.cpu().numpy(), table, cap=cap), "direct call")
        _same(again, FR.find(frames.cpu().numpy(), table, cap=cap), "side stream")
        # the binding's own checks come before any address reaches the library
        with pytest.raises(ValueError, match="connectivity"):
            fb.find(frames, connectivity=5)
        with pytest.raises(ValueError, match="frames of"):
            fb.find(_cuda(np.zeros((1, h, w + 1), np.uint8)))
        with pytest.raises(TypeError, match="GPU"):
            fb.find(frames.cpu())
        with pytest.raises(pt.PdogError, match="table entry 0 is 7"):
            fb.find(frames, [7])
    with pytest.raises(pt.PdogError):
        fb.find(frames)                                                  # closed: a null handle


# ---- track_video(find="frame") ----
def test_track_video_finds_its_targets_in_the_whole_frame(pt, oracle):
    import torch
    tw, args = FS.BOOT_TW, FS.BOOT_ARGS
    video, _ = FS.boot_video()
    cluttered, arena = FS.boot_video(furniture=True)
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    ws = pt.fix_window_size(pt.guess_window_size(tw))
    guesses, kept = FR.start_guesses(video[0], 128, True, tw, 3)
    assert kept == 3
    starts = [tuple(oracle.detect(video[0], 128, K, (ws[0] // 2, ws[1] // 2), g)) for g in guesses]
    runs = {"plain": (video, {}), "background": (cluttered, dict(background=_cuda(arena)))}
    results = {}
    for name, (frames, kw) in runs.items():
        d = _cuda(frames)
        with pytest.raises(ValueError, match="only 0"):                  # the centre window sees none of them
            pt.track_video(d, n_targets=3, find="window", **args, **kw)
        with pytest.raises(ValueError, match="only 0"):
            pt.track_video(d, n_targets=3, **args, **kw)
        ts, idx = pt.track_video(d, n_targets=3, find="frame", **args, **kw)
        got = idx.cpu().numpy()
        assert got.shape == (3, FS.BOOT_NF, 2) and len(ts) == FS.BOOT_NF
        assert [tuple(p) for p in got[:, 0].tolist()] == starts, name   # the restatement's starts: target 0 is the largest disc
        for k in range(FS.BOOT_NF):                                      # and every chain stays on its disc
            assert np.abs(got[:, k] - FS.boot_centres(k)).max() <= 2, (name, k)
        # what a list of those start locations gets
        _, idx2 = pt.track_video(d, start_locations=[("ij", g) for g in guesses], **args, **kw)
        assert torch.equal(idx, idx2)
        results[name] = got
        with pytest.raises(ValueError, match=r"n_targets = 4.*only 3 blob"):
            pt.track_video(d, n_targets=4, find="frame", **args, **kw)
    assert np.array_equal(results["plain"], results["background"])       # the subtracted video IS the clean one
    # on the raw cluttered frames the stain passes for the largest animal: the rule is the restatement's there too
    raw, _ = FR.start_guesses(cluttered[0], int(oracle.mode_u8(cluttered[0])), True, tw, 3)
    _, idx = pt.track_video(_cuda(cluttered), n_targets=3, find="frame", **args)
    got = idx[:, 0].cpu().tolist()
    assert raw[0] == (106, 136) and 101 <= got[0][0] <= 112 and 121 <= got[0][1] <= 150 and [tuple(p) for p in got[1:]] == starts[:2]
    # shape_min_contrast and shape_connectivity are the labelling's: a contrast no disc reaches leaves nothing to find
    with pytest.raises(ValueError, match="only 0 blob"):
        pt.track_video(_cuda(video), n_targets=3, find="frame", shape=True, shape_min_contrast=100, **args)


def test_window_rule_is_what_it_is_without_the_keyword(pt):
    import torch
    nf, h, w = 30, 100, 100
    frames = np.full((nf, h, w), 128, np.uint8)
    yy, xx = np.ogrid[0:h, 0:w]
    for k in range(nf):
        for (ci, cj), v in zip(((41 - k // 5, 41), (41, 59 + k // 5), (59 + k // 4, 50)), (0, 40, 80)):
            frames[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= 4] = v
    d = _cuda(frames)
    args = dict(rate=24, start=0, stop=nf / 24, fps=24, target_width=5, n_targets=3)
    for kw in ({}, dict(subpixel=True), dict(exclusive=True)):
        a, b = pt.track_video(d, **args, **kw), pt.track_video(d, find="window", **args, **kw)
        assert len(a) == len(b) and np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), kw
    assert [tuple(p) for p in a[1][:, 0].cpu().tolist()] != []            # (three starts inside the window)


# ---- the large shapes ----
SCAN_BLOCK, SCAN_PASS = 256, 1024          # pixels per block of the raster, blocks per pass of the scan (dog_frame_blobs.hpp)
T = lambda k: k * (k - 1) // 2  # noqa: E731
S2 = lambda k: (k - 1) * k * (2 * k - 1) // 6  # noqa: E731


@functools.lru_cache(maxsize=None)
def _large_stack(shape):
    """The scenes of one shape of FS.LARGE, drawn once for all the tests below (they do not write to it)."""
    return np.stack([FS.draw(FS.pattern(name, *shape), True, k) for k, name in enumerate(dict(FS.LARGE)[shape])])


@functools.lru_cache(maxsize=None)
def _large_want(shape, conn):
    want = FR.find(_large_stack(shape), connectivity=conn, cap=64)
    for a in want:
        a.setflags(write=False)
    return want


def _full_frame_words(h, w):
    """The one blob of a full mask, in Python integers: the eleven words that do not depend on the contrasts."""
    return [h * w, w * T(h), h * T(w), w * S2(h), T(h) * T(w), h * S2(w), 0, h - 1, 0, w - 1, 0]


@pytest.mark.parametrize("shape", [s for s, _ in FS.LARGE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_shapes_equal_the_restatement_and_the_closed_forms(pt, shape):
    (h, w), names = shape, dict(FS.LARGE)[shape]
    stack = _large_stack(shape)
    k = names.index("full")
    closed = _full_frame_words(h, w)
    assert max(closed) <= 2**63 - 1                                        # an admitted size: the closed forms fit
    with pt.FrameBlobs(h, w, steps_in_flight=2) as fb:                      # every stack takes more than one round
        d = _cuda(stack)
        for conn in (4, 8):
            want = _large_want(shape, conn)
            got = fb.find(d, connectivity=conn, cap=64)
            _same(got, want, (shape, conn))
            count, words = (v.cpu().numpy() for v in got)
            assert count[k].tolist() == [1, h * w]
            assert words[k, 0, :11].tolist() == closed, (shape, conn, words[k, 0].tolist(), closed)
            assert int(words[k, 0, FR.SS]) == int((128 - stack[k].astype(np.int64)).sum()) and not words[k, 1:].any()
            assert int(want[1].max()) > 2**32, (shape, conn)               # the upper halves of the 64-bit words are in use


RANKED = (((520, 520), "checkerboard", 1, 135200), ((1037, 1041), "noise 0.41", 20, 3469), ((1037, 1041), "noise 0.59", 200, 214))


@pytest.mark.parametrize("shape,name,min_area,n_kept", RANKED, ids=[f"{s[0]}x{s[1]} {n}" for s, n, _, _ in RANKED])
def test_kept_blobs_are_ranked_across_every_scan_pass(pt, shape, name, min_area, n_kept):
    h, w = shape
    k = dict(FS.LARGE)[shape].index(name)
    stack = _large_stack(shape)[k:k + 1]
    cap = n_kept + 3
    kw = dict(connectivity=4, min_area=min_area)
    want = FR.find(stack, cap=cap, **kw)
    # what makes this a test of the later passes: the list is not cut, and it has kept blobs in every pass of the scan
    n_passes = ((h * w + SCAN_BLOCK - 1) // SCAN_BLOCK + SCAN_PASS - 1) // SCAN_PASS
    assert want[0][0, 0] == n_kept <= cap and n_passes == {(520, 520): 2, (1037, 1041): 5}[shape]
    passes = want[1][0, :n_kept, FR.FIRST] // SCAN_BLOCK // SCAN_PASS
    assert sorted(set(passes.tolist())) == list(range(n_passes)), np.bincount(passes).tolist()
    assert n_kept > 64 and passes[63] == 0                                  # cap = 64 cuts the list inside the first pass
    with pt.FrameBlobs(h, w, steps_in_flight=2) as fb:
        d = _cuda(stack)
        _same(fb.find(d, cap=cap, **kw), want, (shape, name, cap))         # every row, and the zero rows behind the count
        _same(fb.find(d, cap=64, **kw), (want[0], want[1][:, :64]), (shape, name, 64))


def test_large_shape_behind_a_layout_equals_its_twin(pt):
    shape = (520, 520)
    stack = _large_stack(shape)
    table = [9, 3, 0, 10, 3, 5, 1]                                          # a frame named twice, three rounds and a half
    lay = LF.make(stack, 3, 5, 7, LF.poison_for(True))
    assert lay.row_stride == 523 and lay.base == 5 and lay.frame_stride == 520 * 523 + 7
    with pt.FrameBlobs(*shape, steps_in_flight=2) as fb:
        d, twin = LF.to_device(lay), _cuda(stack)
        for conn in (4, 8):
            want = tuple(a[table] for a in _large_want(shape, conn))
            _same(fb.find(d, table, connectivity=conn, cap=64), want, ("layout", conn))
            _same(fb.find(twin, table, connectivity=conn, cap=64), want, ("twin", conn))


# ---- the largest round ----
def test_the_largest_round_a_handle_holds(pt):
    from pawsometracker_jl_amd import _lib
    h, w, n_steps = 5, 7, 1030
    assert _lib.FB_MAX_IN_FLIGHT == 1024 < n_steps
    stack = FS.noise_frames(0.59, n_steps, h, w)
    assert len({f.tobytes() for f in stack}) == n_steps                     # the steps differ
    d = _cuda(stack)
    want = {conn: FR.find(stack, connectivity=conn, cap=8) for conn in (4, 8)}
    assert len({tuple(c) for c in want[4][0].tolist()}) > 20
    for in_flight in (1024, 1023):                                          # one full round and 6 steps; 1023 and 7
        with pt.FrameBlobs(h, w, steps_in_flight=in_flight) as fb:
            for conn in (4, 8):
                _same(fb.find(d, connectivity=conn, cap=8), want[conn], (in_flight, conn))


# ---- direct calls ----
def _direct(L, fb, frames, table, cap, words_ptr, count_ptr, h, w, conn=8):
    return L.pdog_frame_blobs(fb._h, None, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0],
                              C.c_void_p(table.ctypes.data), len(table), 128, 1, 8, conn, 1, h * w, cap, C.c_void_p(words_ptr), C.c_void_p(count_ptr))


def test_host_table_is_consumed_before_the_call_returns(pt):
    import torch
    from pawsometracker_jl_amd import _lib
    shape = (520, 520)
    stack = _large_stack(shape)
    d = _cuda(stack)
    first = np.array([1, 5, 7, 2, 9], np.int32)
    other = np.array([8, 0, 3, 10, 4], np.int32)
    want = tuple(a[first] for a in _large_want(shape, 8))
    assert not np.array_equal(want[1], _large_want(shape, 8)[1][other])
    words = torch.empty((len(first), 64, 12), dtype=torch.int64, device="cuda")
    count = torch.empty((len(first), 2), dtype=torch.int32, device="cuda")
    with pt.FrameBlobs(*shape, steps_in_flight=2) as fb:
        fb.find(d, connectivity=4)                                          # (the staging has its size; the stream is drained)
        torch.cuda.synchronize()
        assert torch.cuda.current_stream().cuda_stream == 0                 # find and the direct call share the null stream
        fb.find(d, connectivity=8)                                          # work in front of the call: its upload has to wait
        table = first.copy()
        assert _direct(pt.lib(), fb, d, table, 64, words.data_ptr(), count.data_ptr(), *shape) == _lib.PDOG_OK
        table[:] = other                                                    # the caller's array is the caller's again
        torch.cuda.synchronize()
        _same((count, words), want, "table overwritten after return")


def test_outputs_inside_sentinel_margins(pt):
    import torch
    from pawsometracker_jl_amd import _lib
    shape, cap = (520, 520), 64
    stack = _large_stack(shape)
    d = _cuda(stack)
    table = np.arange(len(stack), dtype=np.int32)
    n_words, n_count = len(table) * cap * 12, len(table) * 2
    big_words = torch.full((n_words + 2,), -SENTINEL, dtype=torch.int64, device="cuda")
    big_count = torch.full((n_count + 2,), -SENTINEL, dtype=torch.int32, device="cuda")
    p_words, p_count = big_words.data_ptr() + 8, big_count.data_ptr() + 4
    assert p_words % 16 == 8 and p_count % 16 == 4                          # off a 16-byte boundary, at the natural alignment
    with pt.FrameBlobs(*shape, steps_in_flight=2) as fb:
        for conn in (4, 8):
            assert _direct(pt.lib(), fb, d, table, cap, p_words, p_count, *shape, conn=conn) == _lib.PDOG_OK
            torch.cuda.synchronize()
            _same((big_count[1:-1].view(-1, 2), big_words[1:-1].view(-1, cap, 12)), _large_want(shape, conn), ("margins", conn))
            assert [int(big_words[0]), int(big_words[-1]), int(big_count[0]), int(big_count[-1])] == [-SENTINEL] * 4


# ---- the edges of the admitted sizes ----
def test_sizes_one_past_the_admitted_ones_are_refused_on_the_device(pt):
    from pawsometracker_jl_amd import _lib
    L = pt.lib()
    # (handles of 3 024 617 x 1 and 3 x 2^21, the last admitted ones, are made by the large shapes above)
    assert {(3024617, 1), (3, 1 << 21)} <= {s for s, _ in FS.LARGE}
    for (h, w), text in (((3024618, 1), "Syy"), ((4, 1 << 21), "Sxx"), ((1, (1 << 21) + 1), "PDOG_MAX_ROW_STRIDE")):
        out = C.c_void_p()
        assert L.pdog_fb_create(0, h, w, 1, C.byref(out)) == _lib.PDOG_E_ARG and not out.value
        msg = L.pdog_last_error().decode()
        assert msg.startswith("pdog_fb_create: ") and f"{h} x {w}" in msg and text in msg, msg
        with pytest.raises(ValueError, match=text) as e:
            pt.FrameBlobs(h, w)
        assert f"{h} x {w}" in str(e.value)
