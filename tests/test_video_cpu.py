"""start, stop and fps as host arithmetic (pdog_time_axis, pdog_fps_table) against the exact-rational restatement, the new
symbols' presence and prototypes, and the Python-side checks of a frame table — no GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _args, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_restatement as vr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEO_HDR = os.path.join(ROOT, "include", "pawsome_video.h")
SENTINEL = -77
# (rate, fps) of the stack and of the positions wanted: the pairs for which Float64 and exact arithmetic were compared
PAIRS = [(30, 24), (30, 12), (25, 24), (60, 24), (24, 30), (30, 30), (29.97, 24), (50, 12.5), (30, 7.5)]


def c_time_axis(start, stop, fps, cap=None, want=True):
    """(status, n, ts): ts sentinel-filled with room for cap values (None: as many as the library reports)."""
    n = C.c_int(SENTINEL)
    L = pt.lib()
    if cap is None:
        rc = L.pdog_time_axis(start, stop, fps, None, 0, C.byref(n))
        if rc != _lib.PDOG_OK or not want:
            return rc, n.value, None
        cap = n.value
    ts = np.full(max(cap, 1), float(SENTINEL))
    rc = L.pdog_time_axis(start, stop, fps, C.c_void_p(ts.ctypes.data), cap, C.byref(n))
    return rc, n.value, ts


def c_fps_table(rate, n_frames, start, stop, fps, cap=None):
    n = C.c_int(SENTINEL)
    L = pt.lib()
    if cap is None:
        rc = L.pdog_fps_table(rate, n_frames, start, stop, fps, None, 0, C.byref(n))
        if rc != _lib.PDOG_OK:
            return rc, n.value, None
        cap = n.value
    out = np.full(max(cap, 1), SENTINEL, np.int32)
    rc = L.pdog_fps_table(rate, n_frames, start, stop, fps, C.c_void_p(out.ctypes.data), cap, C.byref(n))
    return rc, n.value, out


def test_video_symbols_are_declared_bound_and_exported():
    hdr = open(VIDEO_HDR).read()
    declared = set(re.findall(r"\b(pdog_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.VIDEO_SYMBOLS) == {"pdog_time_axis", "pdog_fps_table", "pdog_detect_chains_indexed", "pdog_clips_track_indexed"}
    L = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
        fn = getattr(pt.lib(), name)
        restype, argtypes = _lib.VIDEO_PROTOTYPES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert '#include "pawsome_video.h"' in open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
    assert "PDOG_DEFAULT_STOP 86399.999" in hdr and pt.DEFAULT_STOP == 86399.999
    for name in ("time_axis", "fps_table", "track_video"):
        assert callable(getattr(pt, name)), name
    assert hasattr(pt.BatchTracker, "detect_chains_indexed") and hasattr(pt.BatchTracker, "track_clips_indexed")


def test_video_prototype_table_matches_the_header():
    """Argument by argument, as tests/test_abi_cpu.py holds the main table against the main header: an int64_t stride bound as
    c_int would be truncated without a word."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(VIDEO_HDR).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    seen = []
    for stmt in hdr.split(";"):
        m = re.search(r"\bint\s+(pdog_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if not m:
            continue
        restype, argtypes = _lib.VIDEO_PROTOTYPES[m.group(1)]
        seen.append(m.group(1))
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        assert restype is C.c_int and len(args) == len(argtypes), m.group(1)
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (m.group(1), k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (m.group(1), k, decl)
    assert seen == list(_lib.VIDEO_PROTOTYPES)


def test_main_header_alone_declares_the_video_entry_points(tmp_path):
    """A C host includes pawsome_dog.h and nothing else; either header compiles on its own, as C99 and as C++."""
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_dog.h"\n'
                   "int use(double *ts, int32_t *ix, int *n) {\n"
                   "    return pdog_time_axis(0.0, PDOG_DEFAULT_STOP, 24.0, ts, 0, n) + pdog_fps_table(30.0, 10, 0.0, 1.0, 24.0, ix, 0, n);\n}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src)])
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", VIDEO_HDR])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", VIDEO_HDR])


# ---- the time axis ----
TIME_CASES = [(0.0, 1.0, 24.0), (0.2, 1.7, 24.0), (5.0, 60.0, 24.0), (0.0, 86399.999, 24.0), (3.25, 4.75, 30.0), (0.0, 10.0, 0.1),
              (1.0, 2.0, 29.97), (0.0, 0.5, 12.5)]


@pytest.mark.parametrize("start,stop,fps", TIME_CASES)
def test_time_axis_matches_the_restatement(start, stop, fps):
    rc, n, ts = c_time_axis(start, stop, fps)
    assert rc == _lib.PDOG_OK, pt.lib().pdog_last_error()
    assert n == vr.time_axis_len(start, stop, fps)
    assert np.array_equal(ts, vr.time_axis_float(start, stop, fps))          # Float64, operation by operation: the same bits
    tol = vr.time_axis_tolerance(start, stop)
    step = max(1, n // 5000)                                                 # (86399.999 s at 24 fps are 2 M stamps)
    for j in list(range(0, n, step)) + [n - 1]:
        assert abs(vr.Fraction(float(ts[j])) - vr.time_axis_at(start, stop, fps, j)) <= tol, (j, ts[j])
    assert ts[0] == start and (n == 1 or abs(ts[-1] - stop) <= tol)
    assert np.array_equal(pt.time_axis(start, stop, fps), ts)
    for m in (0, 1, 2, n // 2, n - 1, n, n + 5):                            # only the first m stamps (:173): the same bits
        assert np.array_equal(pt.time_axis(start, stop, fps, first=m), ts[:m]), m


def test_time_axis_rounds_ties_to_even_and_handles_one_stamp():
    # fps * t = 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 (refused), 1.5 -> 2: Julia's round(Int, x)
    for start, stop, fps, n_want in ((0.0, 1.0, 2.5, 2), (0.0, 1.0, 3.5, 4), (1.0, 2.0, 4.5, 4), (0.0, 1.0, 1.5, 2), (0.0, 2.0, 2.25, 4)):
        rc, n, ts = c_time_axis(start, stop, fps)
        assert (rc, n) == (_lib.PDOG_OK, n_want) and n == vr.time_axis_len(start, stop, fps), (start, stop, fps, n)
        assert ts[0] == start and abs(ts[-1] - stop) <= vr.time_axis_tolerance(start, stop)
    rc, n, ts = c_time_axis(7.0, 8.0, 1.0)                                   # n = 1: {start}
    assert (rc, n) == (_lib.PDOG_OK, 1) and ts.tolist() == [7.0]
    rc, n, ts = c_time_axis(7.0, 8.0, 1.25)                                  # 1.25 -> 1
    assert (rc, n) == (_lib.PDOG_OK, 1) and ts.tolist() == [7.0]
    assert c_time_axis(0.0, 1.0, 24.0, want=False)[1] == 24                  # a null out_ts only reports n


def test_time_axis_errors_leave_the_outputs_untouched():
    bad = [(1.0, 1.0, 24.0), (2.0, 1.0, 24.0), (0.0, 1.0, 0.0), (0.0, 1.0, -3.0), (0.0, 1.0, 0.5), (0.0, 1.0, 0.25),
           (0.0, float("nan"), 24.0), (0.0, 1.0, float("nan")), (0.0, 1e12, 1e3)]
    for start, stop, fps in bad:
        rc, n, ts = c_time_axis(start, stop, fps, cap=64)
        assert rc == _lib.PDOG_E_ARG and n == SENTINEL and (ts == SENTINEL).all(), (start, stop, fps)
        assert pt.lib().pdog_last_error().startswith(b"pdog_time_axis")
        assert vr.time_axis_len(start, stop, fps) is None or vr.time_axis_len(start, stop, fps) > 2**31 - 1
    rc, n, ts = c_time_axis(0.0, 1.0, 24.0, cap=23)                          # cap < n
    assert rc == _lib.PDOG_E_ARG and n == SENTINEL and (ts == SENTINEL).all()
    assert pt.lib().pdog_time_axis(0.0, 1.0, 24.0, None, 0, None) == _lib.PDOG_E_ARG
    with pytest.raises(pt.PdogError):
        pt.time_axis(1.0, 1.0, 24)


# ---- the fps rule ----
def test_fps_table_examples():
    """The head of three tables: 30 -> 24 drops every fifth frame, 30 -> 12 keeps the later frame of each slot, 24 -> 30 repeats."""
    for rate, fps, head in ((30, 24, [0, 1, 3, 4, 5, 6, 8]), (30, 12, [1, 3, 6, 8, 11]), (24, 30, [0, 1, 1, 2, 3, 4, 5, 5])):
        rc, n, out = c_fps_table(rate, 2000, 0.0, 86399.999, fps)
        assert rc == _lib.PDOG_OK and out[: len(head)].tolist() == head, (rate, fps, out[:10])
        assert vr.fps_table(rate, 2000, 0.0, 86399.999, fps)[: len(head)] == head


@pytest.mark.parametrize("rate,fps", PAIRS)
def test_fps_table_matches_the_restatement(rate, fps):
    """2000 frames; start on a frame time (0, 0.2 s = frame 6 at 30 per second, 0.5), between two (0.21, 1.234); a stop inside
    the stack and the default stop far beyond its end."""
    for start in (0.0, 0.2, 0.21, 0.5, 1.234):
        for stop in (start + 3.0, 86399.999):
            rc, n, out = c_fps_table(rate, 2000, start, stop, fps)
            want = vr.fps_table(rate, 2000, start, stop, fps)
            assert rc == _lib.PDOG_OK and n == len(want), (start, stop, n, len(want))
            assert out.tolist() == want, (start, stop)
            assert np.array_equal(pt.fps_table(rate, 2000, start, stop, fps), out)
            assert (np.diff(out) >= 0).all() and out[0] >= start * rate - 1e-9 and out[-1] <= 1999
            if stop > 2000:                                                  # the stack ends first: fewer outputs than stamps
                assert n < vr.time_axis_len(start, stop, fps) and out[-1] == 1999
            else:
                assert n == vr.time_axis_len(start, stop, fps)


def test_fps_table_small_stacks_and_caps():
    rc, n, out = c_fps_table(30.0, 1, 0.0, 10.0, 24.0)                       # one frame: one output
    assert (rc, n, out.tolist()) == (_lib.PDOG_OK, 1, [0])
    rc, n, out = c_fps_table(30.0, 61, 2.0, 10.0, 30.0)                      # the last frame alone
    assert (rc, n, out.tolist()) == (_lib.PDOG_OK, 1, [60])
    rc, n, out = c_fps_table(30.0, 60, 0.2, 1.7, 24.0, cap=40)               # room to spare: the rest stays untouched
    assert rc == _lib.PDOG_OK and n == 36 and (out[36:] == SENTINEL).all() and out[:36].tolist() == vr.fps_table(30.0, 60, 0.2, 1.7, 24.0)


def test_fps_table_errors_leave_the_outputs_untouched():
    bad = [(0.0, 100, 0.0, 1.0, 24.0), (-30.0, 100, 0.0, 1.0, 24.0), (30.0, 0, 0.0, 1.0, 24.0), (30.0, -5, 0.0, 1.0, 24.0),
           (30.0, 100, -0.1, 1.0, 24.0), (30.0, 100, 1.0, 1.0, 24.0), (30.0, 100, 0.0, 1.0, 0.0), (30.0, 100, 0.0, 1.0, 0.25),
           (30.0, 60, 2.0, 3.0, 24.0),            # frame 60 would be the first at 2 s: the stack ends at 59
           (30.0, 60, 1.99, 3.0, 24.0), (float("nan"), 100, 0.0, 1.0, 24.0), (30.0, 100, float("nan"), 1.0, 24.0)]
    for rate, nf, start, stop, fps in bad:
        rc, n, out = c_fps_table(rate, nf, start, stop, fps, cap=64)
        assert rc == _lib.PDOG_E_ARG and n == SENTINEL and (out == SENTINEL).all(), (rate, nf, start, stop, fps)
        assert pt.lib().pdog_last_error().startswith(b"pdog_fps_table")
        assert vr.fps_table(rate, nf, start, stop, fps) is None
    rc, n, out = c_fps_table(30.0, 100, 0.0, 1.0, 24.0, cap=23)              # cap below the count
    assert rc == _lib.PDOG_E_ARG and n == SENTINEL and (out == SENTINEL).all()
    assert pt.lib().pdog_fps_table(30.0, 100, 0.0, 1.0, 24.0, None, 0, None) == _lib.PDOG_E_ARG
    with pytest.raises(pt.PdogError):
        pt.fps_table(30, 60, start=2.0)


# ---- the binding's own checks ----
def test_frame_table_argument_checks():
    a = _args.host_table([[0, 1, 2], [2, -1, -1]], "frame_table")
    assert a.dtype == np.int32 and a.flags.c_contiguous and a.shape == (2, 3)
    assert _args.host_table(np.arange(12, dtype=np.int64).reshape(3, 4)[:, ::2], "frame_table").tolist() == [[0, 2], [4, 6], [8, 10]]
    import torch
    assert _args.host_table(torch.tensor([[3, 1]]), "frame_table").tolist() == [[3, 1]]
    for exc, v in ((TypeError, [[0.0, 1.0]]), (TypeError, [["a"]]), (ValueError, [0, 1, 2]), (ValueError, np.zeros((2, 0), np.int32)),
                   (ValueError, np.zeros((1, 2, 2), np.int32)), (ValueError, [[2**31]]), (ValueError, [[-2**31 - 1]])):
        with pytest.raises(exc, match="frame_table"):
            _args.host_table(v, "frame_table")


def test_indexed_entry_point_rejects_a_null_tracker():
    tab = np.zeros((1, 2), np.int32)
    rc = pt.lib().pdog_detect_chains_indexed(None, None, 0, 0, 1, C.c_void_p(tab.ctypes.data), 2, 1, 0, None, None)
    assert rc == _lib.PDOG_E_ARG and pt.lib().pdog_last_error().startswith(b"pdog_detect_chains_indexed")
    rc = pt.lib().pdog_clips_track_indexed(None, None, 0, 0, 1, C.c_void_p(tab.ctypes.data), 2, 1, None, 0, None, None)
    assert rc == _lib.PDOG_E_ARG and pt.lib().pdog_last_error().startswith(b"pdog_clips_track_indexed")


def test_indexed_chain_restatement_on_the_oracle(oracle):
    """The restatement itself: over an identity table it is the plain chain, first = 1 keeps the start as given, a row's
    negative tail cuts it, and a repeated frame repeats the fixed point."""
    from oracle import synth
    frames = np.stack([synth.disc_frame(60, 80, (30 + k, 40 + 2 * k), 10, True) for k in range(5)])
    fill = oracle.mode_u8(frames[0])
    args = (10, (21, 21), True)
    plain = vr.chain_indexed(oracle, frames, [0, 1, 2, 3, 4], *args, (30, 40), fill)
    assert plain == [(30 + k, 40 + 2 * k) for k in range(5)]
    assert vr.chain_indexed(oracle, frames, [0, 1, 2, -1, -1], *args, (30, 40), fill) == plain[:3]
    assert vr.chain_indexed(oracle, frames, [-1] * 5, *args, (30, 40), fill) == []
    kept = vr.chain_indexed(oracle, frames, [0, 1, 1, 2], *args, (28, 43), fill, first=1)
    assert kept == [(28, 43), (31, 42), (31, 42), (32, 44)]
    assert vr.chain_indexed(oracle, frames, [4, 3, 2], *args, (34, 48), fill) == [(34, 48), (33, 46), (32, 44)]
