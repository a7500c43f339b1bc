"""pdog_clips_plan (the grouping plan of pdog_clips_track, host arithmetic) against a NumPy restatement, and the new
symbols' presence — no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77
CLIPS_SYMBOLS = ("pdog_clips_create", "pdog_clips_destroy", "pdog_clips_modes", "pdog_clips_plan", "pdog_clips_track")


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def plan(n_clips, n_frames, first, fills, lens):
    """Calls pdog_clips_plan; returns (status, order, group_fill, group_start, n_groups) with sentinel-filled outputs."""
    fa = None if fills is None else np.ascontiguousarray(fills, np.int32)
    la = None if lens is None else np.ascontiguousarray(lens, np.int32)
    cap = max(1, n_clips)
    order = np.full(cap, SENTINEL, np.int32)
    gfill = np.full(min(cap, 256), SENTINEL, np.int32)
    gstart = np.full(min(cap, 256) + 1, SENTINEL, np.int32)
    ng = C.c_int(SENTINEL)
    rc = pt.lib().pdog_clips_plan(n_clips, n_frames, first, _ptr(fa), _ptr(la), _ptr(order), _ptr(gfill), _ptr(gstart), C.byref(ng))
    return rc, order, gfill, gstart, ng.value


def plan_np(n_clips, n_frames, first, fills, lens):
    """The NumPy restatement: participants (len > first) sorted by (fill ascending, len descending, clip ascending)."""
    f = np.full(n_clips, -1, np.int64) if fills is None else np.asarray(fills, np.int64)
    ln = np.full(n_clips, n_frames, np.int64) if lens is None else np.asarray(lens, np.int64)
    clip = np.arange(n_clips)
    keep = ln > first
    f, ln, clip = f[keep], ln[keep], clip[keep]
    o = np.lexsort((clip, -ln, f))          # last key is the primary one
    order, fo = clip[o], f[o]
    starts = [p for p in range(len(order)) if p == 0 or fo[p] != fo[p - 1]]
    return order, fo[starts], np.array(starts + [len(order)])


def check(n_clips, n_frames, first, fills, lens):
    rc, order, gfill, gstart, ng = plan(n_clips, n_frames, first, fills, lens)
    assert rc == _lib.PDOG_OK, pt.lib().pdog_last_error()
    ro, rf, rs = plan_np(n_clips, n_frames, first, fills, lens)
    assert ng == len(rf)
    assert np.array_equal(gstart[: ng + 1], rs)
    assert np.array_equal(gfill[:ng], rf)
    assert np.array_equal(order[: rs[-1]], ro)
    assert (order[rs[-1]:] == SENTINEL).all() and (gfill[ng:] == SENTINEL).all() and (gstart[ng + 1:] == SENTINEL).all()
    # inside a group, the clips still active at frame k are a prefix, for every k
    ln = np.full(n_clips, n_frames) if lens is None else np.asarray(lens)
    for g in range(ng):
        gl = ln[order[gstart[g]:gstart[g + 1]]]
        assert (gl > first).all()
        for k in range(n_frames):
            act = gl > k
            assert not (~act[:-1] & act[1:]).any(), (g, k)
    return order, gfill, gstart, ng


def test_plan_one_clip():
    for first in (0, 1):
        order, gfill, gstart, ng = check(1, 5, first, [17], [5])
        assert ng == 1 and order[0] == 0 and gfill[0] == 17 and list(gstart[:2]) == [0, 1]
    assert check(1, 5, 0, [17], [0])[3] == 0          # nothing to compute: no group
    assert check(1, 1, 1, [17], None)[3] == 0         # first = 1 and one frame: only the copied start, no group


def test_plan_all_fills_equal():
    order, gfill, gstart, ng = check(40, 9, 0, np.full(40, 200), None)
    assert ng == 1 and np.array_equal(order, np.arange(40))


def test_plan_every_fill_distinct():
    rng = np.random.default_rng(0)
    fills = rng.permutation(256)
    order, gfill, gstart, ng = check(256, 4, 0, fills, rng.integers(1, 5, 256))
    assert ng == 256 and np.array_equal(gfill, np.arange(256)) and np.array_equal(fills[order], np.arange(256))


def test_plan_many_clips_three_fills_ragged_lengths():
    rng = np.random.default_rng(1)
    fills = rng.choice([3, 128, 250], 300)
    lens = rng.integers(0, 13, 300)
    for first in (0, 1):
        order, gfill, gstart, ng = check(300, 12, first, fills, lens)
        assert ng == 3
        assert gstart[ng] == int((lens > first).sum())


def test_plan_first_one_drops_lengths_zero_and_one():
    lens = np.array([0, 1, 2, 6, 1, 0, 6, 3])
    order, gfill, gstart, ng = check(8, 6, 1, [9, 9, 9, 9, 4, 4, 4, 4], lens)
    assert list(order[: gstart[ng]]) == [6, 7, 3, 2] and list(gfill[:ng]) == [4, 9] and list(gstart[:3]) == [0, 2, 4]


def test_plan_null_fill_is_one_group_reported_as_minus_one():
    order, gfill, gstart, ng = check(7, 5, 0, None, [5, 0, 3, 5, 1, 2, 4])
    assert ng == 1 and gfill[0] == -1 and list(order[:6]) == [0, 3, 6, 2, 5, 4]


def test_plan_errors_leave_the_outputs_untouched():
    ok_f, ok_l = [1, 2, 3], [4, 4, 4]
    bad = [(0, 4, 0, ok_f, ok_l), (-3, 4, 0, ok_f, ok_l), (3, 0, 0, ok_f, ok_l), (3, -1, 0, ok_f, ok_l),
           (3, 4, 2, ok_f, ok_l), (3, 4, -1, ok_f, ok_l), (3, 4, 0, [1, 256, 3], ok_l), (3, 4, 0, [1, 2, -1], ok_l),
           (3, 4, 0, ok_f, [4, 5, 4]), (3, 4, 1, ok_f, [4, 4, -1])]
    for n_clips, n_frames, first, fills, lens in bad:
        rc, order, gfill, gstart, ng = plan(n_clips, n_frames, first, fills, lens)
        assert rc == _lib.PDOG_E_ARG, (n_clips, n_frames, first, fills, lens)
        assert pt.lib().pdog_last_error().startswith(b"pdog_clips_plan")
        assert (order == SENTINEL).all() and (gfill == SENTINEL).all() and (gstart == SENTINEL).all() and ng == SENTINEL
    # null outputs
    a = np.zeros(4, np.int32)
    ng = C.c_int(SENTINEL)
    L = pt.lib()
    for args in ((None, _ptr(a), _ptr(a), C.byref(ng)), (_ptr(a), None, _ptr(a), C.byref(ng)), (_ptr(a), _ptr(a), None, C.byref(ng)),
                 (_ptr(a), _ptr(a), _ptr(a), None)):
        assert L.pdog_clips_plan(3, 4, 0, None, None, *args) == _lib.PDOG_E_ARG
    assert ng.value == SENTINEL and not a.any()


def test_clips_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
    declared = set(re.findall(r"\b(pdog_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(_lib.LIB_PATH)
    for name in CLIPS_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
        assert getattr(pt.lib(), name).argtypes is not None, name
    assert pt.track_clips is not None and hasattr(pt.BatchTracker, "track_clips") and hasattr(pt.BatchTracker, "clip_modes")


def test_clips_create_rejects_a_null_tracker_with_a_message():
    h = C.c_void_p(1)
    assert pt.lib().pdog_clips_create(None, C.byref(h)) == _lib.PDOG_E_ARG
    assert h.value is None
    assert b"pdog_clips_create" in pt.lib().pdog_last_error()
    assert pt.lib().pdog_clips_create(None, None) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_clips_destroy(None) == _lib.PDOG_OK
    with pytest.raises(pt.PdogError):
        _lib.check(pt.lib().pdog_clips_modes(None, None, 0, 0, 1, None, 1, None))
