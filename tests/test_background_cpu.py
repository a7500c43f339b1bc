"""The background model (include/pawsome_background.h) as far as no GPU is needed: the word arithmetic of csrc/dog_bg_words.hpp
in a stand-alone host program (tests/bg_words_main.cpp, built plain and with AddressSanitizer and UBSan), the sample rule of the
library against the restatement, the header against _lib.BACKGROUND_PROTOTYPES and the library's exports, the Python-side
argument checks, and the two conditions the clutter scene (tests/background_scenes.py) must meet on the Float64 oracle alone:
the plain chain is lost to the hole, the chain on the subtracted frames never is."""
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
import background_restatement as BR  # noqa: E402
import background_scenes as BS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "pawsome_background.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
NAMES = ["pdog_bg_create", "pdog_bg_destroy", "pdog_bg_samples", "pdog_bg_estimate", "pdog_bg_set", "pdog_bg_get", "pdog_bg_subtract_indexed"]


# ---- the word helpers ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_word_helpers_match_a_direct_sort(tmp_path, flags):
    exe = tmp_path / "bg_words"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "bg_words_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert re.search(r"\b[1-9][0-9]* checks, 0 mismatches", p.stdout)


# ---- the sample rule ----
def _lib_samples(table, k, cap=None):
    table = np.ascontiguousarray(table, np.int32)
    out = np.full(64 if cap is None else max(cap, 1), -7, np.int32)
    n = C.c_int(-1)
    rc = pt.lib().pdog_bg_samples(C.c_void_p(table.ctypes.data), len(table), k, C.c_void_p(out.ctypes.data), len(out) if cap is None else cap, C.byref(n))
    return rc, n.value, out


def test_sample_rule_equals_the_restatement():
    rng = np.random.default_rng(11)
    for m in list(range(1, 70)) + [127, 128, 1000, 46341]:
        table = rng.integers(0, 2**31 - 1, m).astype(np.int32)
        for k in (1, 2, 3, 9, 15, 25, 63, 64):
            want = BR.samples(table, k)
            rc, n, out = _lib_samples(table, k)
            assert rc == _lib.PDOG_OK and n == len(want) == min(k, m) and out[:n].tolist() == want and (out[n:] == -7).all(), (m, k)
            assert pt.background_samples(table, k).tolist() == want
    assert BR.samples(range(60), 9) == [0, 6, 13, 20, 26, 33, 40, 46, 53]
    assert BR.samples([5, 5, 2], 64) == [5, 5, 2]                              # k' = m: the table itself, duplicates kept
    # the count alone, too little room, and what is refused
    n = C.c_int(-1)
    tab = np.arange(10, dtype=np.int32)
    assert pt.lib().pdog_bg_samples(C.c_void_p(tab.ctypes.data), 10, 4, None, 0, C.byref(n)) == _lib.PDOG_OK and n.value == 4
    rc, n, out = _lib_samples(tab, 4, cap=3)
    assert rc == _lib.PDOG_E_RANGE and n == 4 and (out == -7).all()
    for args in ((None, 10, 4), (tab, 0, 4), (tab, 10, 0), (tab, 10, 65)):
        p = None if args[0] is None else C.c_void_p(args[0].ctypes.data)
        assert pt.lib().pdog_bg_samples(p, args[1], args[2], C.c_void_p(out.ctypes.data), 64, C.byref(C.c_int())) == _lib.PDOG_E_ARG, args[1:]
        assert pt.lib().pdog_last_error().startswith(b"pdog_bg_samples")
    assert pt.lib().pdog_bg_samples(C.c_void_p(tab.ctypes.data), 10, 4, C.c_void_p(out.ctypes.data), 64, None) == _lib.PDOG_E_ARG


def test_restatement_of_the_rule():
    stack = np.array([[[9, 0]], [[1, 255]], [[5, 0]], [[5, 255]]], np.uint8)           # 4 frames of 1 x 2
    assert BR.median(stack, [0, 1, 2, 3]).tolist() == [[5, 0]]                          # lower median: rank 1 of 4
    assert BR.median(stack, [0, 1, 2]).tolist() == [[5, 0]] and BR.median(stack, [1]).tolist() == [[1, 255]]
    assert BR.median(stack, [0, 0, 1]).tolist() == [[9, 0]]                             # a frame named twice counts twice
    f = np.array([[0, 0, 127, 128, 255, 255, 200]], np.uint8)
    b = np.array([[255, 129, 255, 0, 0, 128, 200]], np.uint8)
    assert BR.subtract(f, b).tolist() == [[0, 0, 0, 255, 255, 255, 128]]
    assert BR.subtract(np.array([[10, 138]], np.uint8), np.array([[138, 10]], np.uint8)).tolist() == [[0, 255]]     # -128 and +128


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


def test_background_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.BACKGROUND_PROTOTYPES) == list(_lib.BACKGROUND_SYMBOLS) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.BACKGROUND_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert len(dict(protos)["pdog_bg_subtract_indexed"]) == 11 and len(dict(protos)["pdog_bg_estimate"]) == 8
    assert "#define PDOG_BG_MAX_SAMPLES 64" in open(HDR).read() and pt.BG_MAX_SAMPLES == _lib.BG_MAX_SAMPLES == BR.MAX_SAMPLES == 64
    main = open(os.path.join(INC, "pawsome_dog.h")).read()
    assert main.index('#include "pawsome_background.h"') > main.index('#include "pawsome_overlay.h"')       # at its end
    assert pt.lib().pdog_abi_version() == 1
    par = inspect.signature(pt.track_video).parameters
    assert par["background"].default is None and par["background_chunk"].default == 256
    for name in ("estimate", "set", "image", "subtract", "close", "__enter__"):
        assert hasattr(pt.Background, name), name
    assert issubclass(pt.Background, _lib.Handle)


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_dog.h"\n'
                   "int use(pdog_bg *b, const uint8_t *f, const int32_t *tab, uint8_t *out, int32_t *idx, int *n) {\n"
                   "    return pdog_bg_samples(tab, 1, PDOG_BG_MAX_SAMPLES, idx, 1, n) + pdog_bg_estimate(b, 0, f, 0, 1, 1, tab, 1)\n"
                   "         + pdog_bg_set(b, 0, f, 1) + pdog_bg_get(b, 0, out, 1) + pdog_bg_subtract_indexed(b, 0, f, 0, 1, 1, tab, 1, out, 1, 1)\n"
                   "         + pdog_bg_destroy(b);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)])
    for hdr in (HDR, os.path.join(INC, "pawsome_dog.h")):
        subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", hdr])
        subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", hdr])


def test_entry_points_refuse_null_arguments_without_a_device():
    L = pt.lib()
    tab = np.zeros(2, np.int32)
    p = C.c_void_p(tab.ctypes.data)
    assert L.pdog_bg_create(0, 4, 4, None) == _lib.PDOG_E_ARG
    h = C.c_void_p(77)
    assert L.pdog_bg_create(0, 0, 4, C.byref(h)) == _lib.PDOG_E_ARG and h.value is None
    assert L.pdog_bg_create(0, 4, -1, C.byref(h)) == _lib.PDOG_E_ARG and L.pdog_last_error().startswith(b"pdog_bg_create")
    assert L.pdog_bg_destroy(None) == _lib.PDOG_OK
    assert L.pdog_bg_estimate(None, None, p, 0, 4, 1, p, 1) == _lib.PDOG_E_ARG and L.pdog_last_error().startswith(b"pdog_bg_estimate")
    assert L.pdog_bg_set(None, None, p, 4) == _lib.PDOG_E_ARG and L.pdog_bg_get(None, None, p, 4) == _lib.PDOG_E_ARG
    assert L.pdog_bg_subtract_indexed(None, None, p, 0, 4, 1, p, 1, p, 16, 4) == _lib.PDOG_E_ARG
    assert L.pdog_last_error().startswith(b"pdog_bg_subtract_indexed")


# ---- the binding's own checks (host tensors: the device is looked at last) ----
def test_python_argument_checks():
    import torch
    for exc, k in ((TypeError, 2.0), (TypeError, True), (TypeError, "9"), (ValueError, 0), (ValueError, 65), (ValueError, -1)):
        with pytest.raises(exc, match="k"):
            _args.background_k(k)
        with pytest.raises(exc):
            pt.background_samples([0, 1, 2], k)
    assert _args.background_k(np.int64(64)) == 64 and _args.background_k(1) == 1
    with pytest.raises(ValueError, match="table"):
        pt.background_samples([], 3)
    with pytest.raises(TypeError, match="table"):
        pt.background_samples([0.5], 3)
    assert _args.host_samples([3, 3, 1], "samples").tolist() == [3, 3, 1]
    for exc, v in ((ValueError, []), (ValueError, list(range(65))), (TypeError, [0.0]), (ValueError, [[0, 1]])):
        with pytest.raises(exc, match="samples"):
            _args.host_samples(v, "samples")
    for exc, hw in ((TypeError, (4.0, 4)), (TypeError, (4, True)), (ValueError, (0, 4)), (ValueError, (4, -2))):
        with pytest.raises(exc, match="frame_"):
            pt.Background(*hw)
    # track_video's keywords are judged before the frames (and those before the device)
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for exc, kw in ((ValueError, dict(background=0)), (ValueError, dict(background=65)), (TypeError, dict(background=2.5)),
                    (TypeError, dict(background=True)), (ValueError, dict(background_chunk=8)),
                    (ValueError, dict(background=3, background_chunk=0)), (TypeError, dict(background=3, background_chunk=1.5))):
        with pytest.raises(exc, match="background") as e:
            pt.track_video(frames, 30, **kw)
        assert type(e.value) is exc, kw
    with pytest.raises(TypeError, match="cuda tensor"):
        pt.track_video(frames, 30, background=3, background_chunk=2)


# ---- the scene, on the oracle alone ----
@pytest.fixture(scope="module")
def oracle():
    from oracle.dog_oracle import Oracle
    return Oracle()


def _plain_chain(oracle, frames, sc):
    from oracle.dog_oracle import OracleTracker
    trk = OracleTracker(frames[0], sc.tw, (sc.ws, sc.ws), sc.darker, oracle)
    track = [trk(sc.starts[0])]
    for f in frames[1:]:
        trk.data[...] = f
        track.append(trk(track[-1]))
    return track


@pytest.mark.parametrize("darker", [True, False], ids=["dark", "bright"])
def test_scene_loses_the_plain_chain_and_keeps_the_subtracted_one(oracle, darker):
    sc = BS.scene(darker)
    err = BS.errors(_plain_chain(oracle, sc.frames, sc), sc.truth[0])
    print("plain: steps off by more than 3 px:", sum(e > 3 for e in err), "last:", err[-1])
    assert sum(e > 3 for e in err) >= 20 and err[-1] > 20
    for K in (9, 15):
        out, _, sub, fill = BR.track_video(oracle, sc.frames, range(sc.nf), K, sc.tw, sc.ws, sc.darker, sc.starts)
        err = BS.errors([tuple(p) for p in out[0]], sc.truth[0])
        print("K =", K, "fill", fill, "worst:", max(err))
        assert max(err) <= 3 and fill == 128
        # the flow is the plain oracle chain on the subtracted frames
        assert [tuple(int(v) for v in p) for p in out[0]] == _plain_chain(oracle, sub, sc)
