"""CPU checks of the diagnostic overlay (src/diagnose.jl): the library's host arithmetic pdog_diag_point against the
restatement, and hand-worked cases of the restatement itself (tests/diag_restatement.py).  No GPU."""
import ctypes as C
import os
import sys

import numpy as np

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_restatement as R  # noqa: E402

SIZES = (100, 240, 271, 320, 481, 720, 1080, 1280, 1920, 2160, 3840)


def test_point_matches_restatement_every_row_and_column():
    L = pt.lib()
    ij, out = (C.c_int32 * 2)(), (C.c_int32 * 2)()
    for n in SIZES:
        for h, w in ((n, 640), (360, n), (n, n)):
            for a in range(1, max(h, w) + 1):
                ij[0], ij[1] = min(a, h), min(a, w)
                assert L.pdog_diag_point(h, w, ij, out) == 0
                assert (out[0], out[1]) == R.point(h, w, (ij[0], ij[1])), (h, w, a)
    assert pt.diag_point(1080, 1920, (1, 1)) == (0, 0)          # rint(1/3): off the buffer
    assert pt.diag_point(1080, 1920, (2, 2)) == (1, 1)
    assert pt.diag_point(2160, 3840, (3, 3)) == (0, 0)          # rint(0.5) = 0, half to even
    assert pt.diag_point(2160, 3840, (9, 9)) == (2, 2)          # rint(1.5) = 2
    assert pt.diag_point(1080, 1920, (1080, 1920)) == (360, 640)
    # outside the frame: clamped into it first
    assert pt.diag_point(1080, 1920, (-7, 5000)) == R.point(1080, 1920, (-7, 5000)) == (0, 640)
    assert pt.diag_point(100, 100, (0, 101)) == (4, 640)


def test_point_bad_arguments():
    L = pt.lib()
    ij, out = (C.c_int32 * 2)(1, 1), (C.c_int32 * 2)()
    assert L.pdog_diag_point(0, 10, ij, out) == _lib.PDOG_E_ARG
    assert L.pdog_diag_point(10, -1, ij, out) == _lib.PDOG_E_ARG
    assert L.pdog_diag_point(10, 10, None, out) == _lib.PDOG_E_ARG
    assert L.pdog_diag_point(10, 10, ij, None) == _lib.PDOG_E_ARG
    assert b"pdog_diag_point" in L.pdog_last_error()


def test_restatement_1080p_is_exact_subsampling():
    img = np.random.default_rng(0).integers(0, 256, (1080, 1920), dtype=np.uint8)
    assert np.array_equal(R.resize(img), img[1::3, 1::3])        # output (I, J) = source (3I-1, 3J-1), 1-based


def test_restatement_4k_is_2x2_mean():
    # 2160 x 3840: every output lands between source rows 6I-3, 6I-2 and columns 6J-3, 6J-2 (1-based), weights 1/2.
    # Sums of 4 that are not 2 mod 4 are not ties: there the byte is the mean rounded to the nearest.
    img = np.random.default_rng(1).integers(0, 64, (2160, 3840), dtype=np.uint8) * 4
    img[2::6, 2::6] += 1                                          # sums are 1 mod 4: no tie anywhere
    s = (img[2::6, 2::6].astype(int) + img[3::6, 2::6] + img[2::6, 3::6] + img[3::6, 3::6])
    assert (s % 4 == 1).all()
    assert np.array_equal(R.resize(img), np.rint(s / 4).astype(np.uint8))


def test_restatement_maps_stay_inside_every_frame():
    for h in SIZES:
        for w in SIZES:
            (i0, i1, fy), (j0, j1, fx) = R.maps(h, w)
            assert i0.min() >= 1 and i1.max() <= h and j0.min() >= 1 and j1.max() <= w
            assert (fy >= 0).all() and (fy < 1).all() and (fx >= 0).all() and (fx < 1).all()


def test_dot_is_the_3x3_block():
    d = R.Diagnose(darker_target=True)
    buf = d(np.zeros((360, 640), np.uint8), (100, 200))
    assert sorted(map(tuple, np.argwhere(buf == 255) + 1)) == [(a, b) for a in (99, 100, 101) for b in (199, 200, 201)]
    d = R.Diagnose(darker_target=False)                        # bright target: drawn in 0
    buf = d(np.full((360, 640), 200, np.uint8), (1, 1))         # clipped at the corner
    assert sorted(map(tuple, np.argwhere(buf == 0) + 1)) == [(1, 1), (1, 2), (2, 1), (2, 2)]


def test_bresenham_direction_changes_the_pixels():
    assert R.segment_pixels((1, 1), (2, 3)) == [(1, 1), (1, 2), (2, 3)]
    assert R.segment_pixels((2, 3), (1, 1)) == [(2, 3), (2, 2), (1, 1)]
    assert R.segment_pixels((0, 0), (2, 2)) == [(1, 1), (2, 2)]          # (0, 0) is off the buffer
    assert R.segment_pixels((5, 5), (5, 5)) == [(5, 5)]


def test_one_point_trace_draws_only_the_dot():
    d = R.Diagnose()
    buf = d(np.zeros((360, 640), np.uint8), (10, 10))
    assert (buf == 255).sum() == 9
    buf = d(np.zeros((360, 640), np.uint8), (10, 20))                 # second point: dot + the segment 10,10 -> 10,20
    assert (buf == 255).sum() == 9 + 11 - 2
    assert len(d.trace) == 2


def test_trace_keeps_the_last_100_points():
    d = R.Diagnose()
    img = np.zeros((360, 640), np.uint8)
    for k in range(150):
        d(img, (1 + k, 1))
    assert len(d.trace) == R.TRACE and d.trace[0] == (51, 1) and d.trace[-1] == (150, 1)
