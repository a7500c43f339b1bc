"""The K-peaks rule (include/pawsome_peaks.h) without a GPU: tests/peaks_restatement.py over hand-made maps — ties,
suppression at and just inside min_distance, the in-frame restriction, shoulders, short outputs —, the four-disc scenes of
tests/test_gpu_peaks.py in both arithmetics (the oracle's Float64 response and the float32 emulation of every kernel
family's pinned order must give the same first four picks: the condition the GPU's comparison with the oracle rests on),
the new header against _lib.PEAKS_PROTOTYPES and the library's exports, and the Python-side argument checks."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _args, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import peaks_restatement as pr  # noqa: E402
import peaks_scenes as ps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAKS_HDR = os.path.join(ROOT, "include", "pawsome_peaks.h")
NINF = np.float32(-np.inf)


def _flat_map(n1, n2, peaks, base=None):
    """An h x w float32 map with value v at window pixel (row, col) for (row, col, v) in peaks.  The background (all below -1)
    falls away from the first of them like a cone, so that it holds no local maximum of its own — a constant `base` has one:
    the plateau's first pixel."""
    yy, xx = np.mgrid[0:n1, 0:n2]
    R = (-1.0 - 0.01 * np.hypot(yy - peaks[0][0], xx - peaks[0][1])).astype(np.float32) if base is None else np.full((n1, n2), base, np.float32)
    for r, c, v in peaks:
        R[r, c] = v
    return R


def _select(R, k, md, guess=None, frame=(1000, 1000), pick1=None):
    """The window centred at `guess` (default: far inside a large frame); pick 1 by default at the map's first maximum."""
    n1, n2 = R.shape
    radii = (n1 // 2, n2 // 2)
    guess = (500, 500) if guess is None else guess
    if pick1 is None:
        i = int(np.nanargmax(R.T.ravel()))
        pick1 = (min(max(guess[0] - radii[0] + i % n1, 1), frame[0]), min(max(guess[1] - radii[1] + i // n1, 1), frame[1]))
    return pr.select(R, guess, radii, frame, pick1, k, md)


def _win(guess, radii, row, col):
    return (guess[0] - radii[0] + row, guess[1] - radii[1] + col)


# ---- the rule over hand-made maps ----
def test_tie_of_two_adjacent_pixels_has_one_local_maximum():
    """Two equal adjacent pixels: only the column-major first is a local maximum — vertically, horizontally and on either
    diagonal; a flat map has exactly one, its first pixel."""
    for (a, b) in (((5, 5), (6, 5)), ((5, 5), (5, 6)), ((5, 5), (6, 6)), ((6, 5), (5, 6))):
        R = _flat_map(11, 11, [(a[0], a[1], 2.0), (b[0], b[1], 2.0)])
        lm = pr.local_maxima(R)
        first = min(a, b, key=lambda p: p[1] * 11 + p[0])
        other = b if first == a else a
        assert lm[first] and not lm[other], (a, b)
    flat = pr.local_maxima(np.zeros((4, 5), np.float32))
    assert flat.sum() == 1 and flat[0, 0]
    nan = np.zeros((5, 5), np.float32)
    nan[2, 2] = np.nan
    assert not pr.local_maxima(nan)[2, 2] and not pr.local_maxima(nan)[1:4, 1:4].any()   # (c), and a NaN neighbour fails (b)


def test_tie_of_two_distant_peaks_goes_to_the_smaller_idx():
    g, radii = (500, 500), (10, 10)
    R = _flat_map(21, 21, [(10, 10, 5.0), (15, 3, 2.0), (2, 16, 2.0), (3, 9, 1.0)])
    ij, peak, count = _select(R, 4, 3)
    assert count == 4
    assert [tuple(p) for p in ij] == [_win(g, radii, 10, 10), _win(g, radii, 15, 3), _win(g, radii, 2, 16), _win(g, radii, 3, 9)]
    assert peak.tolist() == [5.0, 2.0, 2.0, 1.0]      # (15, 3): idx 78 before (2, 16): idx 338, whatever the row
    R2 = _flat_map(21, 21, [(10, 10, 5.0), (2, 3, 2.0), (15, 16, 2.0)])
    assert [tuple(p) for p in _select(R2, 3, 3)[0][1:]] == [_win(g, radii, 2, 3), _win(g, radii, 15, 16)]
    # a positive and a negative zero tie as well
    R3 = _flat_map(21, 21, [(10, 10, 5.0), (15, 3, -0.0), (2, 16, 0.0)])
    ij3, peak3, _ = _select(R3, 3, 3)
    assert tuple(ij3[1]) == _win(g, radii, 15, 3) and np.signbit(peak3[1]) and not np.signbit(peak3[2])


def test_suppression_at_and_just_inside_min_distance():
    """Squared distances in integers: a candidate at exactly min_distance is kept, one at min_distance - 1 dropped — along an
    axis and on the 3-4-5 diagonal —, and an earlier pick other than the first suppresses as well."""
    g, radii = (500, 500), (20, 20)
    md = 5
    for d, kept in ((5, True), (4, False)):
        R = _flat_map(41, 41, [(20, 20, 9.0), (20 + d, 20, 4.0)])
        ij, peak, count = _select(R, 2, md)
        assert (count == 2) == kept and (tuple(ij[1]) == _win(g, radii, 20 + d, 20)) == kept, d
    R = _flat_map(41, 41, [(20, 20, 9.0), (23, 24, 4.0), (17, 17, 3.0)])      # 3-4-5: 25 >= 25 kept; (3, 3): 18 < 25 dropped
    ij, _, count = _select(R, 3, md)
    assert count == 2 and tuple(ij[1]) == _win(g, radii, 23, 24)
    R = _flat_map(41, 41, [(20, 20, 9.0), (30, 30, 4.0), (32, 33, 3.0), (5, 5, 2.0)])  # (32, 33) is 13 < 25 from pick 2 only
    ij, peak, count = _select(R, 4, md)
    assert count == 3 and [tuple(p) for p in ij[:3]] == [_win(g, radii, 20, 20), _win(g, radii, 30, 30), _win(g, radii, 5, 5)]
    assert tuple(ij[3]) == (0, 0) and peak[3] == NINF
    # pick 1 suppresses at its CLAMPED position, not at the window pixel that held the maximum
    frame, guess = (100, 100), (3, 50)                 # window rows -17 … 23: the maximum in the padding, row -5
    R = _flat_map(41, 41, [(12, 20, 9.0), (20 + 3, 20, 4.0), (20 + 8, 20, 3.0)])
    ij, _, count = pr.select(R, guess, radii, frame, (1, 50), 3, md)
    assert [tuple(p) for p in ij[:count]] == [(1, 50), (6, 50), (11, 50)]     # rows 6 and 11: 5 and 10 from row 1 — and 5 apart


def test_a_larger_value_in_the_padding_is_never_picked():
    frame, radii = (60, 80), (10, 10)
    guess = (5, 78)                                     # window rows -5 … 15, columns 68 … 88: frame rows 1 …, columns … 80
    R = _flat_map(21, 21, [(2, 3, 50.0), (8, 18, 40.0), (12, 5, 3.0), (15, 9, 2.0), (6, 12, 1.0)])
    # (2, 3) is frame row -3, (8, 18) is frame column 86: both outside; pick 1 as the functor clamps the maximum's position
    ij, peak, count = pr.select(R, guess, radii, frame, (1, 71), 4, 2)
    assert peak[0] == 50.0 and tuple(ij[0]) == (1, 71)            # the window's maximum, padding included
    assert [tuple(p) for p in ij[1:count]] == [(7, 73), (10, 77), (1, 80)] and count == 4
    assert peak[1:].tolist() == [3.0, 2.0, 1.0]
    # a window wholly beside the frame on one axis: no candidate at all
    assert pr.select(R, (30, 200), radii, frame, (30, 80), 4, 2)[2] == 1


def test_a_shoulder_outside_the_disc_is_not_a_pick():
    """A bright peak's flank just outside the suppression disc beats every true secondary peak in value, but it is not a local
    maximum, so it is no candidate."""
    n = 41
    yy, xx = np.mgrid[0:n, 0:n]
    R = (100.0 - 4.0 * np.hypot(yy - 20, xx - 20)).astype(np.float32)      # a cone: at distance 6 still 76
    R[5, 33] = 60.0                                                         # the true second peak, on the cone's flank (value there ~ 23)
    ij, peak, count = _select(R, 2, 6)
    assert count == 2 and tuple(ij[1]) == _win((500, 500), (20, 20), 5, 33) and peak[1] == 60.0
    assert R[20, 26] > 60.0 and not pr.local_maxima(R)[20, 26]


def test_short_output_is_padded():
    R = _flat_map(15, 15, [(7, 7, 3.0), (2, 2, 1.0), (12, 3, 0.5)])
    ij, peak, count = _select(R, 6, 2)
    assert pr.local_maxima(R).sum() == 3
    assert count == 3 and (ij[3:] == 0).all() and (peak[3:] == NINF).all() and ij.dtype == np.int32 and peak.dtype == np.float32
    assert pr.default_min_distance(10) == 10 and pr.default_min_distance(9.2) == 10 and pr.default_min_distance(0.3) == 1
    one = _select(R, 1, 2)
    assert one[2] == 1 and one[0].shape == (1, 2)


# ---- the four-disc scenes in both arithmetics ----
@pytest.mark.parametrize("name", list(ps.SCENES))
def test_scenes_agree_in_both_arithmetics(oracle, name):
    """The rule over the oracle's Float64 response and over the float32 emulation of each family's pinned order: the first
    four picks are the disc centres in contrast order in every one of them."""
    sc = ps.scene(name)
    K = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    assert K.shape[0] == sc.l == 29
    pos, R64 = oracle.detect(sc.frame, sc.fill, K, sc.radii, sc.guess, want_resp=True)
    md = pr.default_min_distance(sc.tw)
    want = [tuple(c) for c in sc.centres]
    ij, peak, count = pr.select(R64, sc.guess, sc.radii, sc.hw, pos, 6, md)
    assert count >= 4 and [tuple(p) for p in ij[:4]] == want, (name, "float64", ij[:count])
    assert (np.diff(peak[:4]) < 0).all() and peak[3] > 0
    tile = fr.window_tile(sc.frame, sc.fill, sc.l, sc.radii, sc.guess)
    for family in fr.FAMILIES:
        R32 = fr.response_f32(tile, sc.fill, sc.tw, True, family, n1=sc.ws[0], n2=sc.ws[1])
        assert R32.dtype == np.float32 and R32.shape == R64.shape
        first = int(np.argmax(R32.T.ravel()))
        p1 = (sc.guess[0] - sc.radii[0] + first % sc.ws[0], sc.guess[1] - sc.radii[1] + first // sc.ws[0])
        ij32, peak32, c32 = pr.select(R32, sc.guess, sc.radii, sc.hw, p1, 6, md)
        assert c32 >= 4 and [tuple(p) for p in ij32[:4]] == want, (name, family, ij32[:c32])
        # the margin the agreement has: the picks' values lie far further apart than the two arithmetics do
        assert np.abs(R32.astype(np.float64) - R64).max() < 1e-5 < -np.diff(peak[:4]).max() / 100


def test_scene_geometry():
    for name in ps.SCENES:
        sc = ps.scene(name)
        assert sc.hw == (120, 160) and sc.tw == 10 and sc.fill == 128 and sorted(sc.values) == [0, 30, 60, 90]
        c = np.array(sc.centres)
        d2 = ((c[:, None] - c[None]) ** 2).sum(-1) + np.eye(4, dtype=int) * 10**6
        assert d2.min() >= 25 * 25
        lo = np.array(sc.guess) - np.array(sc.radii)
        assert (c - 5 >= np.maximum(lo, 1)).all() and (c + 5 <= np.minimum(lo + np.array(sc.ws) - 1, sc.hw)).all()
        assert [int(sc.frame[i - 1, j - 1]) for i, j in sc.centres] == [0, 30, 60, 90]


# ---- the header, the table, the exports ----
def _prototypes(path):
    hdr = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    out = []
    for stmt in hdr.split(";"):
        m = re.search(r"\bint\s+(pdog_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            out.append((m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]))
    return out


def test_peaks_symbols_are_declared_bound_and_exported():
    protos = _prototypes(PEAKS_HDR)
    assert [name for name, _ in protos] == list(_lib.PEAKS_PROTOTYPES) == ["pdog_detect_peaks", "pdog_get_peaks_counts"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.PEAKS_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert len(dict(protos)["pdog_detect_peaks"]) == 14
    hdr = open(PEAKS_HDR).read()
    assert "#define PDOG_PEAKS_MAX_K 32" in hdr and _lib.PEAKS_MAX_K == pr.MAX_K == 32
    assert pt.lib().pdog_abi_version() == 1          # an addition: the version stays, as for the earlier headers
    src = open(os.path.join(ROOT, "pawsometracker.jl_amd", "csrc", "dog_peaks.hpp")).read()
    assert f"PEAKS_LIST = {pr.LIST_CAPACITY};" in src
    assert hasattr(pt.BatchTracker, "detect_peaks") and hasattr(pt.BatchTracker, "peaks_counts")
    par = inspect.signature(pt.track_video).parameters
    assert par["n_targets"].default is None and par["min_distance"].default is None
    assert list(inspect.signature(pt.BatchTracker.detect_peaks).parameters)[1:] == ["frames", "guesses", "k", "min_distance", "frame_index", "want_resp"]


def test_header_compiles_alone(tmp_path):
    for cc, flags in (("gcc", ["-x", "c", "-std=c99", "-Wextra"]), ("g++", ["-x", "c++"])):
        subprocess.check_call([cc] + flags + ["-fsyntax-only", "-Wall", "-Werror", PEAKS_HDR])
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_peaks.h"\n'
                   "int use(pdog_tracker *t, const uint8_t *f, const int32_t *g, int32_t *ij, float *pk, int32_t *cnt) {\n"
                   "    return pdog_detect_peaks(t, f, 0, 0, 1, 0, g, 1, PDOG_PEAKS_MAX_K, 0, ij, pk, cnt, 0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_null_and_range_arguments_are_refused_without_a_device():
    """What pdog_detect_peaks judges before it touches a tracker: no GPU needed."""
    L = pt.lib()
    assert L.pdog_detect_peaks(None, None, 0, 0, 1, None, None, 1, 3, 0, None, None, None, None) == _lib.PDOG_E_ARG
    assert b"null tracker" in L.pdog_last_error()
    out = (C.c_uint64 * 2)()
    assert L.pdog_get_peaks_counts(None, out) == _lib.PDOG_E_ARG


def test_python_arguments_are_checked():
    assert _args.peaks_args(3, None) == (3, 0) and _args.peaks_args(np.int64(32), 7) == (32, 7)
    for exc, k, md in ((TypeError, 2.0, None), (TypeError, True, None), (TypeError, "3", None), (ValueError, 0, None),
                       (ValueError, 33, None), (TypeError, 3, 2.5), (TypeError, 3, True), (ValueError, 3, 0), (ValueError, 3, -4)):
        with pytest.raises(exc) as e:
            _args.peaks_args(k, md)
        assert type(e.value) is exc and re.search(r"k|min_distance", str(e.value)), (k, md)
    import torch
    frames = torch.zeros((2, 40, 40), dtype=torch.uint8)
    with pytest.raises(ValueError, match="not both"):           # judged before anything touches the device
        pt.track_video(frames, 24, n_targets=2, start_locations=[None, None])
    with pytest.raises(ValueError, match="n_targets"):
        pt.track_video(frames, 24, n_targets=33)
    with pytest.raises(TypeError, match="n_targets"):
        pt.track_video(frames, 24, n_targets=2.0)
    with pytest.raises(ValueError, match="min_distance"):
        pt.track_video(frames, 24, min_distance=5)
