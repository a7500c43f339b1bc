"""The layout tests have teeth, shown on the oracle alone (no GPU).

tests/test_gpu_layout.py hands every detection kernel the scenes of tests/layout_frames.py behind strided, offset,
overlapping and aliased layouts and demands the contiguous twin's bits.  That only catches a kernel that misreads a layout
if the misreading CHANGES an answer.  Here every scene, in the worst corner of the layout matrix (odd slack, odd base, odd
gap), is misread in each of the four ways layout_frames.misreadings states — the pitch taken as w, the frame stride taken
as h*row_stride, the base dropped, slack and gap bytes read where the fill belongs — and the oracle's position must change
in at least one window of the scene.  A scene that cannot see a misreading must be changed, not the test.
Also: the argument checks let each of these views through up to the device check, and the two host-side readers of strided
frames (pdog_mode_u8, pdog_window_tile) agree with the contiguous twin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_frames as lf  # noqa: E402


def test_make_builds_what_it_says():
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (3, 6, 10), dtype=np.uint8)
    for slack, base, gap in ((0, 0, 0), (1, 5, 0), (19, 2 * 10 + 5, 3 * 10 + 7), (64, 13, 7)):
        lay = lf.make(frames, slack, base, gap, 5)
        v = lay.view
        assert v.strides == (6 * (10 + slack) + gap, 10 + slack, 1) and np.array_equal(v, frames) and np.array_equal(lay.twin(), frames)
        assert v.__array_interface__["data"][0] - lay.flat.__array_interface__["data"][0] == base
        mask = np.ones(lay.flat.size, bool)                       # every byte outside the frames holds the poison
        for k in range(3):
            for i in range(6):
                a = base + k * lay.frame_stride + i * lay.row_stride
                mask[a:a + 10] = False
        assert (lay.flat[mask] == 5).all() and mask[-lf.TAIL:].all()
    tall = rng.integers(0, 256, (2 * 4 + 6, 10), dtype=np.uint8)
    ov = lf.overlapping(tall, 3, 6, 4, 3, 7, 250)
    assert ov.frame_stride == 4 * 13 and np.array_equal(ov.view[2], tall[8:14]) and np.array_equal(ov.view[1][4:], ov.view[2][:2])
    al = lf.aliased(frames[0], 4, 1, 3, 5)
    assert al.frame_stride == 0 and all(np.array_equal(al.view[k], frames[0]) for k in range(4))
    # the misreadings differ from the truth exactly where the layout differs from the contiguous one
    mis = lf.misreadings(lf.make(frames, 19, 25, 37, 5), 77)
    assert all(not np.array_equal(mis[m][:, :6, :10], frames) for m in lf.MISREADINGS[:3])
    ext = mis[lf.MISREADINGS[3]]
    assert ext.shape == (3, 12, 20) and (ext[:, :6, 10:] == 5).all() and (ext[:2, 6, :] == 5).all() and (ext[2, 10:] == 77).all()
    ext = lf.misreadings(lf.make(frames, 3, 25, 0, 5), 77)[lf.MISREADINGS[3]]      # behind the slack the next row, below the frame the next one
    assert (ext[:, :6, 10:13] == 5).all() and np.array_equal(ext[0, :5, 13:], frames[0, 1:, :7]) and np.array_equal(ext[0, 6:, :10], frames[1])
    same = lf.misreadings(lf.make(frames, 0, 0, 0, 5), 77)
    assert all(np.array_equal(same[m], frames) for m in lf.MISREADINGS[:3])


@pytest.mark.parametrize("name,content", lf.USED)
def test_every_scene_catches_every_misreading(oracle, name, content):
    sc = lf.scene(name, content)
    lay = sc.worst()
    assert lay.row_stride % 2 == 1 or sc.w % 2 == 1
    assert lay.base % 2 == 1 and lay.frame_stride % lay.row_stride != 0
    K = sc.kernel(oracle)
    # every launch holds: a window inside the frame, one over each border, one over a corner
    r1, r2 = sc.radii
    gs = [g for _, g in sc.windows]
    assert any(g[0] - r1 < 1 for g in gs) and any(g[0] + r1 > sc.h for g in gs) and any(g[1] - r2 < 1 for g in gs) and any(g[1] + r2 > sc.w for g in gs)
    assert any(g[0] - r1 >= 1 and g[0] + r1 <= sc.h for g in gs)
    for what, frames in lf.misreadings(lay, sc.fill).items():
        changed = 0
        for k, g in sc.windows:
            if lf.misread_position(oracle, frames[k], sc.h, sc.w, sc.fill, K, sc.radii, g) != sc.position(oracle, k, g):
                changed += 1
                break
        assert changed, (name, content, what)


@pytest.mark.parametrize("name", ["l29 21x21", "l65 45x45"])
def test_overlapping_and_aliased_frames_are_seen(oracle, name):
    """The two extra layouts: taking the frame stride for h*row_stride changes an overlapping stack's answers, and an
    aliased stack's twin really is nf copies of one frame (so any non-zero frame stride reads something else: the poison)."""
    sc = lf.scene(name)
    ov = lf.overlap_of(sc)
    twin = ov.twin()
    wrong = lf.misreadings(ov, sc.fill)[lf.MISREADINGS[1]]
    assert any(tuple(oracle.detect(wrong[k], sc.fill, sc.kernel(oracle), sc.radii, g)) != sc.position(oracle, k, g, twin, "overlap")
               for k, g in sc.windows if k > 0)
    al = lf.alias_of(sc)
    assert al.frame_stride == 0 and all(np.array_equal(f, sc.frames[0]) for f in al.twin())


def test_argument_checks_let_every_layout_through():
    """_args.device_frames on host tensors of each layout: everything about them is in order but the device (see
    test_argument_helpers_reject_bad_input for what it refuses)."""
    import torch
    from pawsometracker_jl_amd import _args
    sc = lf.scene("l29 21x21 odd w")
    hw = (sc.h, sc.w)
    lays = [lf.make(sc.frames, s, b, g, sc.poison) for s, b, g in lf.matrix(sc)[::7] + lf.diagonal(sc)] + [lf.overlap_of(sc), lf.alias_of(sc)]
    for lay in lays:
        t = lf.host_tensor(lay)
        assert t.stride() == (lay.frame_stride, lay.row_stride, 1) and np.array_equal(t.numpy(), lay.view)
        with pytest.raises(TypeError, match="must live on the GPU"):
            _args.device_frames(t, "frames", 3, hw)
    lay = lf.make(np.concatenate([sc.frames, sc.frames[:1]]), 19, 2 * sc.w + 5, 3 * sc.w + 7, sc.poison)      # four frames as two clips of two
    t4 = torch.as_strided(torch.from_numpy(lay.flat), (2, 2, sc.h, sc.w), (2 * lay.frame_stride, lay.frame_stride, lay.row_stride, 1), lay.base)
    with pytest.raises(TypeError, match="must live on the GPU"):
        _args.device_frames(t4, "frames", 4, hw)
    with pytest.raises(ValueError, match="stacked contiguously"):
        _args.device_frames(torch.as_strided(t4, t4.shape, (2 * lay.frame_stride + 1, lay.frame_stride, lay.row_stride, 1), lay.base), "frames", 4, hw)
    # a crop on a plain tensor is such a view too
    big = torch.zeros((3, sc.h + 3, sc.w + 5), dtype=torch.uint8)
    crop = big[:, 3:, 5:]
    assert crop.stride() == (big.stride(0), sc.w + 5, 1) and crop.storage_offset() == 3 * (sc.w + 5) + 5
    with pytest.raises(TypeError, match="must live on the GPU"):
        _args.device_frames(crop, "frames", 3, hw)


def test_the_binding_knows_the_headers_bound():
    import re
    from pawsometracker_jl_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pawsome_dog.h")).read()
    m = re.search(r"#define PDOG_MAX_ROW_STRIDE \(1 << (\d+)\)", hdr)
    assert m and _lib.PDOG_MAX_ROW_STRIDE == 1 << int(m.group(1)) == 1 << 21


def test_host_readers_agree_with_the_contiguous_twin(oracle):
    """pdog_mode_u8 and pdog_window_tile (host code, no GPU) over a frame of each layout against the contiguous twin."""
    import pawsometracker_jl_amd as pt
    L = pt.lib()
    sc = lf.scene("l29 21x21 odd w")
    hw = sc.l // 2
    th, tww = 2 * sc.radii[0] + sc.l, 2 * sc.radii[1] + sc.l
    for s, b, g in lf.matrix(sc)[::5] + lf.diagonal(sc):
        lay = lf.make(sc.frames, s, b, g, sc.poison)
        view, twin = lay.view, lay.twin()
        for k in range(sc.nf):
            m, m2 = C.c_int(), C.c_int()
            assert L.pdog_mode_u8(view[k].ctypes.data, sc.h, sc.w, lay.row_stride, C.byref(m)) == 0
            assert L.pdog_mode_u8(twin[k].ctypes.data, sc.h, sc.w, sc.w, C.byref(m2)) == 0
            assert m.value == m2.value == oracle.mode_u8(twin[k])
            for guess in sc.by_frame[k]:
                gg = (C.c_int32 * 2)(*guess)
                a, c = np.full((th, tww + 3), 9, np.uint8), np.full((th, tww + 3), 9, np.uint8)
                assert L.pdog_window_tile(view[k].ctypes.data, sc.h, sc.w, lay.row_stride, sc.fill, float(sc.tw), sc.ws[0], sc.ws[1], gg, a.ctypes.data, tww + 3) == 0
                assert L.pdog_window_tile(twin[k].ctypes.data, sc.h, sc.w, sc.w, sc.fill, float(sc.tw), sc.ws[0], sc.ws[1], gg, c.ctypes.data, tww + 3) == 0
                assert np.array_equal(a, c) and np.array_equal(a[:, :tww], lf.fr.window_tile(twin[k], sc.fill, sc.l, sc.radii, guess)), (s, b, g, k, guess)
    assert hw > 0
