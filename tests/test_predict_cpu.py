"""The predicted chain (include/pawsome_predict.h) without a GPU: tests/predict_restatement.py against tests/motion_restatement.py
at T = 1, k = 1 — on the "fast" and "vanish" scenes of tests/motion_scenes.py and on seeded random lists with a v that
overflows, an n_held at INT32_MAX, NaN peaks and peaks equal to min_response —, the two scenes as the feature's issue asks
them to come out, the rule's header under the host compiler, the new header against _lib.PREDICT_PROTOTYPES and the library's
exports, and the Python-side argument checks."""
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
import motion_restatement as mr  # noqa: E402
import motion_scenes as ms  # noqa: E402
import predict_restatement as prs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pawsome_predict.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
HW = (ms.H, ms.W)


# ---- the restatement equals the motion rule for one target and one pick ----
def test_restatement_equals_the_motion_rule_on_random_lists():
    """4000 seeded steps: positions in and around the frame, velocities small or at the ends of int32 (p + v and p' - p overflow
    32 bits), n_held small, at the coast or at INT32_MAX, peaks from a handful of values with NaN, -inf, +inf, both zeros and
    the threshold itself; min_ratio 0, 0.5 and 1 (an infinite peak fails 0 * inf, which no finite response can reach)."""
    rng = np.random.default_rng(20261020)
    kinds = set()
    for n in range(4000):
        coast = int(rng.integers(0, 5))
        m = [0.0, 0.25, 1e-3][n % 3]
        p = rng.integers(-3, 150, 2)
        v = rng.integers(-9, 10, 2)
        nh = int(rng.integers(0, 6))
        if n % 5 == 0:
            v = np.where(rng.integers(0, 2, 2) == 1, 2**31 - 1 - rng.integers(0, 3, 2), -2**31 + rng.integers(0, 3, 2))
        if n % 7 == 0:
            p = np.where(rng.integers(0, 2, 2) == 1, 2**31 - 1 - rng.integers(0, 3, 2), -2**31 + rng.integers(0, 3, 2))
        if n % 4 == 0:
            nh = 2**31 - 1 - int(rng.integers(0, 2))
        R = np.float32([m, np.nan, -np.inf, 0.0, -0.0, 0.5, np.nextafter(np.float32(m), np.float32(1)), 3.0, 1e-3, -1.0][int(rng.integers(0, 10))])
        q = rng.integers(1, 141, 2)
        mstate = np.array([v[0], v[1], nh, int(rng.integers(0, 99))], np.int64)
        got = prs.step(p, mstate, R, q, HW, m, coast)
        for rho in (1.0, 0.5, 0.0):
            want = mr.step(p[None], mstate[None], q[None, None].astype(np.int32), np.array([[R]], np.float32), np.array([int(rng.integers(0, 3))]),
                           HW, int(rng.integers(1, 20)), rho, m, coast)
            assert tuple(want[0][0]) == got[0] and int(want[1][0]) == got[1] and tuple(want[2][0]) == got[2], (n, p, mstate, R, q, m, coast)
            assert np.array_equal(want[3][0], got[3]), (n, p, mstate, R, m, coast)
        kinds.add((got[1], bool(R != R), bool(R == np.float32(m)), nh >= 2**31 - 2, n % 5 == 0))
    assert {(-1, True, False), (-1, False, True), (1, False, False)} <= {k[:3] for k in kinds}
    assert any(k[3] and k[0] == -1 for k in kinds) and any(k[4] for k in kinds)
    # +inf: the motion rule with min_ratio 0 forms 0 * inf; with min_ratio 1 — what the library's fallback passes — it is assigned
    inf = mr.step(np.array([[5, 5]]), np.zeros((1, 4), np.int64), np.array([[[7, 7]]], np.int32), np.array([[np.inf]], np.float32), np.array([1]), HW, 3, 1.0, 0.0, 2)
    assert int(inf[1][0]) == 1 == prs.step((5, 5), np.zeros(4), np.float32(np.inf), (7, 7), HW, 0.0, 2)[1]


@pytest.fixture(scope="module")
def walks(oracle):
    out = {}
    for name in ("fast", "vanish"):
        sc = ms.scene(name)
        Kn = oracle.dog_kernel(oracle.sigma(sc.tw), True)
        out[name] = prs.walk(oracle, sc.frames, sc.fill, Kn, sc.radii, np.arange(sc.nf), sc.starts[0], sc.min_response, sc.coast, first=1)
    return out


@pytest.mark.parametrize("name", ["fast", "vanish"])
def test_restatement_equals_the_motion_walk_on_the_scenes(oracle, walks, name):
    sc = ms.scene(name)
    assert sc.k == 1 and len(sc.starts) == 1
    track, states, _, contested = ms.walk_float64(oracle, sc)
    out, state, _ = walks[name]
    assert [tuple(int(v) for v in p) for p in out] == [t[0] for t in track]
    assert state.tolist() == [0] + [s[0] for s in states] and not any(c[0] for c in contested)


def test_fast_target_in_a_small_window(oracle, walks):
    sc = ms.scene("fast")
    out, state, mstate = walks["fast"]
    track = [[tuple(int(v) for v in p)] for p in out]
    errs = ms.errors_true(track, sc.truth)
    print("fast at 11 x 11: worst error", max(errs), "steps above 3 px:", ms.steps_above_true(track, sc.truth))
    assert max(errs) <= 3 and (state[1:] == 1).all() and mstate.tolist() == [0, ms.FAST_SPEED, 0, 0]
    plain = ms.plain_chain_float64(oracle, sc)                                 # the premise: the plain chain does not
    assert ms.steps_above_true(plain, sc.truth) >= 13


def test_vanished_target_coasts_and_stops(walks):
    sc = ms.scene("vanish")
    out, state, mstate = walks["vanish"]
    assert [tuple(int(v) for v in p) for p in out[ms.VANISH_FROM:]] == ms.VANISH_TAIL
    assert state.tolist() == [0] + [1] * (ms.VANISH_FROM - 1) + [-1] * (sc.nf - ms.VANISH_FROM)
    assert mstate.tolist() == [0, 0, sc.nf - ms.VANISH_FROM, 0]


def test_walk_over_a_table(oracle):
    """first = 0 files step 0 from the start; a row's negative tail is not walked; a clip without a step keeps its mstate; a walk
    split in two equals the one-call walk."""
    sc = ms.scene("vanish")
    Kn = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    args = (oracle, sc.frames, sc.fill, Kn, sc.radii)
    row = np.array(list(range(1, 14)) + [-1, -1])
    one = prs.walk(*args, row, sc.truth[0][0], 1e-3, 3)
    assert (one[0][13:] == 0).all() and (one[1][13:] == 0).all() and one[1][0] == 1 and tuple(one[0][0]) == (50, 20)      # from rest: the window's edge, 2 px short
    a = prs.walk(*args, row[:10], sc.truth[0][0], 1e-3, 3)
    b = prs.walk(*args, row[10:], a[0][-1], 1e-3, 3, mstate=a[2])
    assert np.array_equal(np.concatenate([a[0], b[0]]), one[0]) and np.array_equal(np.concatenate([a[1], b[1]]), one[1]) and np.array_equal(b[2], one[2])
    given = np.array([3, -4, 5, 6], np.int32)
    assert np.array_equal(prs.walk(*args, np.array([-1, -1]), (5, 5), 0.0, 3, mstate=given)[2], given)
    assert np.array_equal(prs.walk(*args, np.array([4, -1]), (5, 5), 0.0, 3, first=1, mstate=given)[2], given)


# ---- the rule's header under the host compiler, with the sanitizers ----
MAIN = r'''
#include "pdog_predict.hpp"
#include <cstdio>
using namespace pdog::predict;
int main()
{
    int bad = 0;
    Walk w{50, 15, {0, 0, 0}};
    Filed f = step(w, assigned(0.1f, 0.f), 50, 15, 50, 22, 3, 100, 140);           // assigned: v' = p' - p
    bad += !(f.i == 50 && f.j == 22 && f.state == 1 && f.gi == 50 && f.gj == 29 && w.c.vj == 7 && w.c.n_held == 0);
    f = step(w, assigned(0.f, 0.f), 50, 29, 1, 1, 2, 100, 140);                      // 0 does not exceed 0: held, coasts
    bad += !(f.i == 50 && f.j == 29 && f.state == -1 && f.gj == 36 && w.c.n_held == 1 && w.c.vj == 7);
    f = step(w, assigned(__builtin_nanf(""), 0.f), 50, 36, 1, 1, 2, 100, 140);      // a NaN fails; n_held' = coast: at rest
    bad += !(f.state == -1 && f.gj == 36 && w.c.n_held == 2 && w.c.vj == 0);
    Walk e{2147483647, -2147483647 - 1, {2147483647, -2147483647 - 1, 2147483647}};  // nothing overflows
    bad += !(predict(e.pi, e.c.vi, 100) == 100 && predict(e.pj, e.c.vj, 140) == 1);
    f = step(e, false, 100, 1, 0, 0, 5, 100, 140);
    bad += !(e.c.n_held == 2147483647 && e.c.vi == 0 && f.i == 100 && f.j == 1);
    e.pi = -2147483647 - 1;
    f = step(e, true, 100, 1, 7, 9, 5, 100, 140);                                    // p' - p wraps modulo 2^32
    bad += !(e.c.vi == -2147483641 && e.c.vj == 8 && f.state == 1 && e.pi == 7);
    std::printf("%d mismatches\n", bad);
    return bad != 0;
}
'''


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_rule_header_as_a_program(tmp_path, flags):
    tu = tmp_path / "predict_main.cpp"
    tu.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(tu), "-o", str(tmp_path / "predict")])
    p = subprocess.run([str(tmp_path / "predict")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr


# ---- the header, the table, the exports (fails on a library without the feature) ----
def _prototypes(path):
    hdr = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    out = []
    for stmt in hdr.split(";"):
        m = re.search(r"\bint\s+(pdog_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            out.append((m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]))
    return out


def test_predict_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.PREDICT_PROTOTYPES) == ["pdog_detect_chains_predicted", "pdog_get_predict_counts"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.PREDICT_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert [len(a) for _, a in protos] == [15, 2]
    assert pt.lib().pdog_abi_version() == 1          # an addition: the version stays
    # a null tracker is judged before anything else: no GPU needed
    assert pt.lib().pdog_detect_chains_predicted(None, None, 0, 0, 1, None, 1, 1, 0, 0.0, 2, None, None, None, None) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_get_predict_counts(None, (C.c_uint64 * 4)()) == _lib.PDOG_E_ARG
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pawsome_predict.h" in mk and "$(O)/pawsome_predict.o" in mk
    # the kernels include the rule's header, which takes the clamp and the carries from the motion rule's
    assert '#include "pdog_predict.hpp"' in open(os.path.join(CSRC, "dog_roll.hpp")).read()
    assert '#include "dog_roll.hpp"' in open(os.path.join(CSRC, "dog_fused.hpp")).read()
    assert '#include "pdog_motion.hpp"' in open(os.path.join(CSRC, "pdog_predict.hpp")).read()
    earlier = set(_lib.PROTOTYPES) | set(_lib.PEAKS_PROTOTYPES) | set(_lib.EXCLUSIVE_PROTOTYPES) | set(_lib.MOTION_PROTOTYPES)
    assert not set(_lib.PREDICT_PROTOTYPES) & earlier
    par = inspect.signature(pt.track_video).parameters
    assert par["predict"].default is False and list(par).index("predict") < list(par).index("motion")
    sig = inspect.signature(pt.BatchTracker.detect_chains_predicted).parameters
    assert list(sig)[1:] == ["frames", "frame_table", "starts", "min_response", "coast", "mstate", "first"]
    assert (sig["min_response"].default, sig["coast"].default, sig["mstate"].default, sig["first"].default) == (0.0, 8, None, 0)


def test_header_compiles_alone():
    for cc, flags in (("gcc", ["-x", "c", "-std=c99", "-Wextra"]), ("g++", ["-x", "c++"])):
        subprocess.check_call([cc] + flags + ["-fsyntax-only", "-Wall", "-Werror", HDR])


def test_python_arguments_are_checked():
    """Raised before the library is touched: the tensors live on the host, and the handle is no tracker at all."""
    assert _args.predict_args(0, 0) == (0.0, 0) and _args.predict_args(0.5, 8) == (0.5, 8)
    for exc, a in ((ValueError, (-1e-9, 8)), (ValueError, (float("nan"), 8)), (ValueError, (float("inf"), 8)), (ValueError, (1e39, 8)),
                   (TypeError, ("0", 8)), (TypeError, (True, 8)), (TypeError, (None, 8)), (ValueError, (0.0, -1)), (TypeError, (0.0, 2.0)),
                   (TypeError, (0.0, True)), (TypeError, (0.0, None)), (ValueError, (0.0, 2**31))):
        with pytest.raises(exc) as e:
            _args.predict_args(*a)
        assert type(e.value) is exc, a
    import torch
    bt = pt.BatchTracker.__new__(pt.BatchTracker)          # no tracker behind it: whatever reached the library would fail loudly
    bt._h, bt._hw, bt.use_torch_stream = None, (40, 40), lambda: None
    frames, starts, table = torch.zeros((3, 40, 40), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32), [[0, 1, 2], [0, 1, -1]]
    for exc, call in ((ValueError, lambda: bt.detect_chains_predicted(frames, table, starts, coast=-1)),
                      (TypeError, lambda: bt.detect_chains_predicted(frames, table, starts, coast=1.0)),
                      (ValueError, lambda: bt.detect_chains_predicted(frames, table, starts, min_response=-1)),
                      (ValueError, lambda: bt.detect_chains_predicted(frames, table, starts, min_response=float("nan"))),
                      (ValueError, lambda: bt.detect_chains_predicted(frames, table, starts, first=2)),
                      (TypeError, lambda: bt.detect_chains_predicted(frames, [[0.5]], starts)),
                      (ValueError, lambda: bt.detect_chains_predicted(frames, [0, 1], starts)),
                      (TypeError, lambda: bt.detect_chains_predicted(frames.float(), table, starts)),
                      (ValueError, lambda: bt.detect_chains_predicted(frames[:, :30], table, starts)),
                      (TypeError, lambda: bt.detect_chains_predicted(frames, table, starts))):                     # host tensors: the device is judged last
        with pytest.raises(exc):
            call()
    for kw, exc, match in ((dict(predict=True, motion=True), ValueError, "predict"), (dict(predict=True, exclusive=True), ValueError, "predict"),
                           (dict(predict=1), TypeError, "predict"), (dict(predict=True, coast=-1), ValueError, "coast"),
                           (dict(predict=True, coast=1.5), TypeError, "coast"), (dict(predict=True, min_response=-1.0), ValueError, "min_response"),
                           (dict(predict=True, min_ratio=0.5), ValueError, "min_ratio"), (dict(predict=True, min_distance=5), ValueError, "min_distance"),
                           # what held without the keyword holds with it
                           (dict(coast=3), ValueError, "coast"), (dict(min_response=0.1), ValueError, "min_response"),
                           (dict(motion=True, exclusive=True), ValueError, "exclusive")):
        with pytest.raises(exc, match=match):                      # judged before anything touches the device
            pt.track_video(frames, 24, **kw)
