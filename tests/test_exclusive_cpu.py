"""The exclusive step (include/pawsome_exclusive.h) without a GPU: tests/exclusive_restatement.py over hand-made lists — T = 1,
a shared pick 1, the ratio's edge, short counts, -inf entries, value ties, blocking by a later assignment, a held target inside
another's distance —, the library's host function against the restatement on seeded random groups, the same function as a
stand-alone program under AddressSanitizer and UBSan, the two scenes of tests/exclusive_scenes.py over the oracle's Float64
maps (independent chains collapse, the exclusive walk keeps one target on each disc), the new header against
_lib.EXCLUSIVE_PROTOTYPES and the library's exports, and the Python-side argument checks."""
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
import exclusive_restatement as er  # noqa: E402
import exclusive_scenes as es  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pawsome_exclusive.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
NINF = -np.inf


def _step(prev, lists, d=10, rho=0.5):
    """lists[t] = [((row, col), value), ...]; count = the list's length, padded to the longest with (0, 0) and -inf."""
    k = max(len(l) for l in lists)
    ij = np.zeros((len(lists), k, 2), np.int32)
    peak = np.full((len(lists), k), NINF, np.float32)
    for t, l in enumerate(lists):
        for q, (p, v) in enumerate(l):
            ij[t, q], peak[t, q] = p, v
    out, state = er.assign(np.array(prev, np.int32), ij, peak, np.array([len(l) for l in lists], np.int32), d, rho)
    return [tuple(int(v) for v in p) for p in out], state.tolist()


# ---- the rule over hand-made lists ----
def test_one_target_takes_pick_one():
    assert _step([(5, 5)], [[((20, 30), 1.0), ((40, 40), 0.9)]]) == ([(20, 30)], [1])
    assert _step([(5, 5)], [[((20, 30), NINF)]]) == ([(20, 30)], [1])              # whatever its value: the functor
    assert _step([(5, 5)], [[((20, 30), -3.0), ((40, 40), 5.0)]]) == ([(20, 30)], [1])   # list order, not value order


def test_two_targets_with_the_same_pick_one():
    """The stronger view of the shared blob wins it; the other takes its pick 2 if that is admissible and is held otherwise."""
    shared = (50, 60)
    out, st = _step([(48, 55), (52, 66)], [[(shared, 2.0), ((50, 30), 1.5)], [(shared, 3.0), ((50, 90), 2.0)]])
    assert (out, st) == ([(50, 30), shared], [2, 1])
    out, st = _step([(48, 55), (52, 66)], [[(shared, 2.0), ((50, 30), 0.5)], [(shared, 3.0)]])
    assert (out, st) == ([(48, 55), shared], [-1, 1])                                # 0.5 < 0.5 * 2.0: held at prev
    # pick 1 positions that differ but lie within d count as the same blob
    out, st = _step([(48, 55), (52, 66)], [[((50, 60), 2.0)], [((55, 68), 3.0)]])
    assert (out, st) == ([(48, 55), (55, 68)], [-1, 1])                              # 25 + 64 < 100
    out, st = _step([(48, 55), (52, 66)], [[((50, 60), 2.0)], [((56, 68), 3.0)]])
    assert (out, st) == ([(50, 60), (56, 68)], [1, 1])                               # 36 + 64 = 100, exactly d: free


def test_pick_two_below_and_exactly_at_the_ratio():
    """rho_f * peak[0] is one float32 product: 0.7f * 0.7f rounds to 0.48999998, below the double product 0.49 — a value AT the
    float32 product is admissible though double arithmetic would refuse it; one ulp below it is not."""
    rho, v0 = 0.7, np.float32(0.7)
    edge = np.float32(rho) * v0
    below = np.nextafter(edge, np.float32(0))
    assert edge.dtype == np.float32 and float(edge) < rho * float(v0) and float(edge) < 0.49
    shared = (50, 60)
    for v, want in ((edge, 2), (below, -1), (np.float32(0.49), 2)):
        _, st = _step([(1, 1), (2, 2)], [[(shared, v0), ((10, 10), v)], [(shared, 4.0)]], rho=rho)
        assert st == [want, 1], (v, st)
    # rho = 0 admits every positive value, none at or below zero; rho = 1 only a tie with pick 1
    for v, rho, want in ((1e-30, 0.0, 2), (0.0, 0.0, -1), (-1.0, 0.0, -1), (2.999, 1.0, -1), (3.0, 1.0, 2)):
        _, st = _step([(1, 1), (2, 2)], [[(shared, 3.0), ((10, 10), v)], [(shared, 4.0)]], rho=rho)
        assert st == [want, 1], (v, rho, st)
    # a negative pick 1 admits no pick 2, though the ratio test alone would pass
    assert _step([(1, 1), (2, 2)], [[(shared, -3.0), ((10, 10), -1.0)], [(shared, 4.0)]])[1] == [-1, 1]


def test_count_below_k_and_infinite_entries():
    shared = (50, 60)
    ij = np.array([[shared, (10, 10), (90, 90)], [shared, (0, 0), (0, 0)]], np.int32)
    peak = np.array([[2.0, 1.8, 1.7], [3.0, NINF, NINF]], np.float32)
    prev = np.array([(1, 1), (2, 2)], np.int32)
    for count0, want in ((3, 2), (2, 2), (1, -1), (0, -1)):
        out, st = er.assign(prev, ij, peak, np.array([count0, 1], np.int32), 10, 0.5)
        assert st.tolist() == [want, 1] and tuple(out[0]) == ((10, 10) if want == 2 else (1, 1)), count0
    # -inf entries inside the count are not admissible, an entry behind them is
    peak2 = np.array([[2.0, NINF, 1.7], [3.0, NINF, NINF]], np.float32)
    out, st = er.assign(prev, ij, peak2, np.array([3, 3], np.int32), 10, 0.5)
    assert st.tolist() == [3, 1] and tuple(out[0]) == (90, 90)
    # a window of NaNs reports -inf for pick 1: still pick 1, ranked last
    out, st = _step([(1, 1), (2, 2)], [[(shared, NINF)], [((51, 61), -5.0)]])
    assert st == [-1, 1]


def test_exact_value_ties_go_to_the_smaller_target():
    shared = (50, 60)
    out, st = _step([(1, 1), (2, 2), (3, 3)], [[(shared, 2.0)], [(shared, 2.0)], [(shared, 2.0)]])
    assert st == [1, -1, -1] and out == [shared, (2, 2), (3, 3)]
    out, st = _step([(1, 1), (2, 2)], [[(shared, -0.0)], [(shared, 0.0)]])           # the two zeros tie
    assert st == [1, -1]
    out, st = _step([(1, 1), (2, 2)], [[(shared, 2.0), ((10, 10), 1.5)], [(shared, 2.0), ((90, 90), 1.9)]])
    assert (out, st) == ([shared, (90, 90)], [1, 2])


def test_an_entry_blocked_by_the_second_assignment_only():
    """Target 2's pick 1 falls to target 0 (round 1), its pick 2 is free of that position but falls to target 1 (round 2): it
    ends on pick 3."""
    a, b = (50, 60), (50, 90)
    out, st = _step([(1, 1), (2, 2), (3, 3)], [[(a, 5.0)], [(b, 4.0)], [((52, 61), 3.0), ((51, 92), 2.9), ((20, 20), 2.0)]])
    assert (out, st) == ([a, b, (20, 20)], [1, 1, 3])
    # list order decides, not value: an unsorted list offers its weaker, earlier entry first
    out, st = _step([(1, 1), (2, 2)], [[(a, 5.0)], [((52, 61), 3.0), ((20, 20), 1.6), ((80, 20), 2.9)]])
    assert (out, st) == ([a, (20, 20)], [1, 2])


def test_a_held_target_blocks_nobody():
    """Target 1 is held at prev (55, 62), within d of target 0's assigned position and of target 2's: both are assigned."""
    out, st = _step([(49, 58), (55, 62), (60, 64)], [[((50, 60), 5.0)], [((50, 60), 4.0)], [((60, 66), 3.0)]])
    assert (out, st) == ([(50, 60), (55, 62), (60, 66)], [1, -1, 1])
    assert (55 - 50) ** 2 + (62 - 60) ** 2 < 100 and (55 - 60) ** 2 + (62 - 66) ** 2 < 100


# ---- the host function against the restatement ----
def _host(prev, ij, peak, count, d, rho):
    G, T, k = peak.shape
    out = np.full((G, T, 2), 777, np.int32)
    state = np.full((G, T), 777, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = pt.lib().pdog_assign_exclusive_host(G, T, k, d, rho, P(prev), P(ij), P(peak), P(count), P(out), P(state))
    return rc, out, state


def random_groups(rng, G, T, k, grid, wild_values=True):
    """Positions on a grid x grid lattice (blocking is common), values from a handful of levels (ties are common) with -inf,
    NaN and both zeros among them, unsorted, counts 0 ... k + 1."""
    prev = rng.integers(0, grid, (G, T, 2)).astype(np.int32)
    ij = rng.integers(0, grid, (G, T, k, 2)).astype(np.int32)
    peak = ((rng.integers(0, 9, (G, T, k)) - 2) * 0.25).astype(np.float32)
    if wild_values:
        kind = rng.integers(0, 16, (G, T, k))
        peak[kind == 0] = NINF
        peak[kind == 1] = np.nan
        peak[kind == 2] = -0.0
    count = rng.integers(0, k + 2, (G, T)).astype(np.int32)
    return prev, ij, peak, count


def test_host_function_equals_the_restatement_on_random_groups():
    rng = np.random.default_rng(20251019)
    n_groups = blocked = held = later = 0
    for trial in range(700):
        T, k = (1 + trial % 32, 32 - trial % 32) if trial < 64 else (int(rng.integers(1, 33)), int(rng.integers(1, 33)))
        G, d, grid = int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 14))
        rho = [0.0, 1.0, 0.5][trial % 3] if trial % 4 == 0 else float(rng.integers(0, 1001)) / 1000.0
        prev, ij, peak, count = random_groups(rng, G, T, k, grid)
        rc, out, state = _host(prev, ij, peak, count, d, rho)
        assert rc == _lib.PDOG_OK
        want, wstate = er.assign_groups(prev, ij, peak, count, d, rho)
        assert np.array_equal(state, wstate) and np.array_equal(out, want), (trial, T, k, d, rho, state, wstate)
        n_groups += G
        held += int((wstate == -1).sum())
        later += int((wstate > 1).sum())
    assert n_groups > 1000 and held > 1000 and later > 1000      # the draw exercises what it is for


def test_host_function_refuses_bad_arguments():
    prev, ij, peak, count = random_groups(np.random.default_rng(1), 1, 2, 3, 5)
    ok = dict(G=1, T=2, k=3, d=4, rho=0.5)
    L = pt.lib()
    P = lambda a: C.c_void_p(a.ctypes.data)
    out, state = np.full((1, 2, 2), 9, np.int32), np.full((1, 2), 9, np.int32)
    for kw in (dict(G=0), dict(T=0), dict(T=33), dict(k=0), dict(k=33), dict(d=0), dict(d=-1), dict(rho=-0.01), dict(rho=1.01),
               dict(rho=float("nan"))):
        a = dict(ok, **kw)
        assert L.pdog_assign_exclusive_host(a["G"], a["T"], a["k"], a["d"], a["rho"], P(prev), P(ij), P(peak), P(count), P(out), P(state)) == _lib.PDOG_E_ARG, kw
        assert L.pdog_last_error() != b""
    for null in range(6):
        ptrs = [P(prev), P(ij), P(peak), P(count), P(out), P(state)]
        ptrs[null] = None
        assert L.pdog_assign_exclusive_host(1, 2, 3, 4, 0.5, *ptrs) == _lib.PDOG_E_ARG
    assert (out == 9).all() and (state == 9).all()
    # the device entry points judge a null tracker before anything else: no GPU needed
    assert L.pdog_assign_exclusive(None, 1, 2, 3, 4, 0.5, None, None, None, None, None, None) == _lib.PDOG_E_ARG
    assert L.pdog_detect_chains_exclusive(None, None, 0, 0, 1, None, 1, 1, 1, 0, 0, 0, 0.5, None, None, None) == _lib.PDOG_E_ARG
    assert L.pdog_get_exclusive_counts(None, (C.c_uint64 * 2)()) == _lib.PDOG_E_ARG


# ---- the stand-alone program, plain and under the sanitizers ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_host_function_as_a_program(tmp_path, flags):
    exe = tmp_path / "exclusive"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "exclusive_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout


def test_rule_header_compiles_alone(tmp_path):
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "pdog_exclusive.hpp"\nint main() { return pdog::exclusive::admissible(0, 0, 0.f, 0.f, 0.f) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(tu), "-o", str(tmp_path / "alone")])


# ---- the two scenes over the oracle's Float64 maps ----
@pytest.fixture(scope="module")
def walks(oracle):
    return {name: es.walk_float64(oracle, es.scene(name)) for name in es.SCENES}


@pytest.mark.parametrize("name", list(es.SCENES))
def test_scenes_in_float64(walks, name):
    sc = es.scene(name)
    ind, exc, states = walks[name]
    truth = sc.truth
    # the premise: independent chains end on ONE disc
    assert ind[-1][0] == ind[-1][1] and ind[-1][0] in truth[-1], (name, ind[-1])
    if name == "passing":                                          # ("through": which of two mirror-equal discs is a last-bit matter)
        assert ind[-1] == [(44, 110), (44, 110)]                   # the weak target's chain jumped to the strong one
    # the exclusive walk ends with one target exactly on each disc
    assert sorted(exc[-1]) == sorted(truth[-1]), (name, exc[-1])
    if name == "passing":
        assert exc[-1] == truth[-1]                                # identities kept
        assert {1, 2, -1} <= {s for st in states for s in st}
    d2 = es.min_assigned_distance2(exc, states)
    assert d2 is not None and d2 >= es.MIN_DISTANCE ** 2
    errs = es.errors(exc, truth)
    print(name, "steps above 3 px:", es.steps_above(exc, truth), "worst:", max(errs), "states:", sorted({s for st in states for s in st}))
    assert es.steps_above(exc, truth) <= es.FLOAT64_STEPS_ABOVE_3PX[name]
    assert es.steps_above(ind, truth) >= 20                        # what a collapse costs


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


def test_exclusive_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.EXCLUSIVE_PROTOTYPES) == [
        "pdog_assign_exclusive", "pdog_assign_exclusive_host", "pdog_detect_chains_exclusive", "pdog_get_exclusive_counts"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.EXCLUSIVE_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert [len(a) for _, a in protos] == [12, 11, 16, 2]
    hdr = open(HDR).read()
    assert "#define PDOG_EXCLUSIVE_MAX_TARGETS 32" in hdr and _lib.EXCLUSIVE_MAX_TARGETS == er.MAX_TARGETS == 32
    assert pt.lib().pdog_abi_version() == 1          # an addition: the version stays, as for the earlier headers
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pawsome_exclusive.h" in mk and "$(O)/pawsome_exclusive.o" in mk
    # the kernel and the host function share the rule's header
    for unit in ("dog_assign.hpp", "pdog_math.cpp"):
        assert '#include "pdog_exclusive.hpp"' in open(os.path.join(CSRC, unit)).read(), unit
    par = inspect.signature(pt.track_video).parameters
    assert list(par)[-2:] == ["exclusive", "min_ratio"] and par["exclusive"].default is False and par["min_ratio"].default is None
    assert list(inspect.signature(pt.BatchTracker.assign_exclusive).parameters)[1:] == ["prev", "ij", "peak", "count", "min_distance", "min_ratio"]
    sig = inspect.signature(pt.BatchTracker.detect_chains_exclusive).parameters
    assert list(sig)[1:] == ["frames", "frame_table", "starts", "k", "min_distance", "min_ratio", "first"]
    assert sig["min_ratio"].default == 0.5 and sig["first"].default == 0 and sig["k"].default is None


def test_header_compiles_alone(tmp_path):
    for cc, flags in (("gcc", ["-x", "c", "-std=c99", "-Wextra"]), ("g++", ["-x", "c++"])):
        subprocess.check_call([cc] + flags + ["-fsyntax-only", "-Wall", "-Werror", HDR])


def test_python_arguments_are_checked():
    assert _args.exclusive_args(2, None, None, 0.5) == (0, 0, 0.5) and _args.exclusive_args(32, 4, 7, 1) == (4, 7, 1.0)
    for exc, a in ((ValueError, (0, None, None, 0.5)), (ValueError, (33, None, None, 0.5)), (ValueError, (2, 0, None, 0.5)),
                   (ValueError, (2, 33, None, 0.5)), (TypeError, (2, 2.0, None, 0.5)), (ValueError, (2, 2, 0, 0.5)),
                   (TypeError, (2, 2, 1.5, 0.5)), (ValueError, (2, 2, None, -0.1)), (ValueError, (2, 2, None, 1.1)),
                   (ValueError, (2, 2, None, float("nan"))), (TypeError, (2, 2, None, "0.5")), (TypeError, (2, 2, None, True)),
                   (TypeError, (2, 2, None, None))):
        with pytest.raises(exc) as e:
            _args.exclusive_args(*a)
        assert type(e.value) is exc, a
    import torch
    frames = torch.zeros((2, 40, 40), dtype=torch.uint8)
    with pytest.raises(ValueError, match="min_ratio"):           # judged before anything touches the device
        pt.track_video(frames, 24, min_ratio=0.5)
    with pytest.raises(ValueError, match="min_ratio"):
        pt.track_video(frames, 24, exclusive=True, min_ratio=1.5)
    with pytest.raises(TypeError, match="exclusive"):
        pt.track_video(frames, 24, exclusive=1)
    with pytest.raises(ValueError, match="n_targets"):
        pt.track_video(frames, 24, exclusive=True, start_locations=[None] * 33)
    with pytest.raises(ValueError, match="min_distance"):
        pt.track_video(frames, 24, min_distance=5)               # still belongs to n_targets or exclusive
