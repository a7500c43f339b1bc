"""The motion step (include/pawsome_motion.h) without a GPU: tests/motion_restatement.py over hand-made lists — nearest to the
prediction instead of pick 1, a weak pick 1, D ties, blocking by a later assignment, contested and uncontested velocities,
coasting, clamping, the saturation of D —, the library's host function against the restatement on seeded random groups, the
same function as a stand-alone program under AddressSanitizer and UBSan, the four scenes of tests/motion_scenes.py over the
oracle's Float64 maps, the new header against _lib.MOTION_PROTOTYPES and the library's exports, and the Python-side argument
checks."""
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
import exclusive_scenes as es  # noqa: E402
import motion_restatement as mr  # noqa: E402
import motion_scenes as ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pawsome_motion.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
NINF = -np.inf
HW = (100, 140)


def _step(prev, lists, v=None, n_held=None, d=10, rho=0.5, m=0.0, coast=8, hw=HW):
    """lists[t] = [((row, col), value), ...]; count = the list's length, padded to the longest with (0, 0) and -inf.  Returns
    (positions, states, next guesses, [(v_row, v_col, n_held)])."""
    T, k = len(lists), max(1, max(len(l) for l in lists))
    ij = np.zeros((T, k, 2), np.int32)
    peak = np.full((T, k), NINF, np.float32)
    for t, l in enumerate(lists):
        for q, (p, val) in enumerate(l):
            ij[t, q], peak[t, q] = p, val
    mstate = np.zeros((T, 4), np.int64)
    mstate[:, :2] = v if v is not None else 0
    mstate[:, 2] = n_held if n_held is not None else 0
    out, state, nxt, new = mr.step(np.array(prev, np.int64), mstate, ij, peak, np.array([len(l) for l in lists], np.int32), hw, d, rho, m, coast)
    assert (new[:, 3] == 0).all()
    tup = lambda a: [tuple(int(x) for x in p) for p in a]
    return tup(out), state.tolist(), tup(nxt), tup(new[:, :3])


# ---- the rule over hand-made lists ----
def test_one_target_takes_the_entry_nearest_to_its_prediction():
    far, near = ((20, 30), 1.0), ((52, 63), 0.9)
    # at rest the prediction is prev: pick 2 is nearer
    assert _step([(50, 60)], [[far, near]])[:2] == ([(52, 63)], [2])
    # moving by (-10, -10) per step the prediction (40, 50) is still nearer to pick 2 (313 against 800) ...
    assert _step([(50, 60)], [[far, near]], v=[(-10, -10)])[:2] == ([(52, 63)], [2])
    # ... and by (-25, -25) it is nearer to pick 1: (25, 35), 50 against 1513
    out, st, nxt, new = _step([(50, 60)], [[far, near]], v=[(-25, -25)])
    assert (out, st) == ([(20, 30)], [1]) and new == [(-30, -30, 0)] and nxt == [(1, 1)]      # v' = p' - p; the guess is clamped
    # an equal D goes to the smaller q, whatever the values
    assert _step([(50, 60)], [[((50, 57), 0.5), ((50, 63), 0.9)]])[:2] == ([(50, 57)], [1])
    # the ratio counts as in the exclusive rule: a near entry below rho * pick 1 is not offered
    assert _step([(50, 60)], [[far, ((52, 63), 0.4)]])[:2] == ([(20, 30)], [1])
    # an entry at or beyond the count is not offered, entry 0 is whatever the count says
    assert mr.step([(50, 60)], [[0, 0, 0, 0]], [[(20, 30), (52, 63)]], [[1.0, 0.9]], [1], HW, 10, 0.5, 0.0, 8)[1].tolist() == [1]
    assert mr.step([(50, 60)], [[0, 0, 0, 0]], [[(20, 30), (52, 63)]], [[1.0, 0.9]], [0], HW, 10, 0.5, 0.0, 8)[1].tolist() == [1]


def test_pick_one_at_or_below_min_response_leaves_the_target_held():
    for val, m, want in ((0.0, 0.0, -1), (-0.0, 0.0, -1), (1e-30, 0.0, 1), (1e-3, 1e-3, -1), (np.nextafter(np.float32(1e-3), np.float32(1)), 1e-3, 1),
                         (NINF, 0.0, -1), (np.nan, 0.0, -1), (-2.0, 0.0, -1)):
        out, st, nxt, new = _step([(50, 60)], [[((50, 61), val)]], v=[(0, 2)], m=m)
        assert st == [want], (val, m, st)
        if want == -1:                                            # held: the prediction is filed, the velocity kept
            assert out == [(50, 62)] and new == [(0, 2, 1)] and nxt == [(50, 64)]
    # min_response is compared as a float32: 0.1 (double) rounds UP to float32(0.1), which the value float32(0.1) does not exceed
    assert _step([(50, 60)], [[((50, 61), np.float32(0.1))]], m=0.1)[1] == [-1]
    # a NaN pick 1 fails the ratio test of every later entry too
    assert _step([(50, 60)], [[((50, 61), np.nan), ((50, 62), 1.0)]])[1] == [-1]
    # an empty window (count 0, -inf) offers nothing
    assert _step([(50, 60)], [[]])[:2] == ([(50, 60)], [-1])


def test_equal_distances_go_to_the_larger_value_then_to_the_smaller_target():
    shared = (50, 60)
    # both predictions 5 columns from the shared blob
    out, st, _, _ = _step([(50, 55), (50, 65)], [[(shared, 2.0)], [(shared, 3.0)]])
    assert (out, st) == ([(50, 55), shared], [-1, 1])
    out, st, _, _ = _step([(50, 55), (50, 65), (45, 60)], [[(shared, 2.0)], [(shared, 2.0)], [(shared, 2.0)]])
    assert st == [1, -1, -1]
    # (no zero and no NaN ever competes: neither exceeds a min_response >= 0)
    assert _step([(50, 55), (50, 65)], [[(shared, -0.0)], [(shared, 0.0)]])[1] == [-1, -1]
    # the nearer target wins whatever the values: D decides first
    out, st, _, _ = _step([(50, 56), (50, 65)], [[(shared, 2.0)], [(shared, 9.0)]])
    assert (out, st) == ([shared, (50, 65)], [1, -1])
    # the loser of a tie goes on to its next nearest entry
    out, st, _, _ = _step([(50, 55), (50, 65)], [[(shared, 2.0), ((50, 30), 1.5)], [(shared, 2.0), ((50, 90), 1.9)]])
    assert (out, st) == ([shared, (50, 90)], [1, 2])


def test_an_entry_blocked_by_a_later_assignment():
    """Target 2's nearest entry falls to target 0 (round 1), its next nearest to target 1 (round 2): it ends on its farthest."""
    a, b = (50, 60), (50, 90)
    out, st, _, _ = _step([(50, 60), (50, 90), (53, 62)], [[(a, 5.0)], [(b, 4.0)], [((52, 61), 3.0), ((51, 88), 2.9), ((20, 20), 2.0)]])
    assert (out, st) == ([a, b, (20, 20)], [1, 1, 3])
    # with nothing left it is held at its prediction and blocks nobody
    out, st, _, _ = _step([(50, 60), (50, 90), (53, 62)], [[(a, 5.0)], [(b, 4.0)], [((52, 61), 3.0), ((51, 88), 2.9)]])
    assert (out, st) == ([a, b, (53, 62)], [1, 1, -1])
    # exactly d away is free
    out, st, _, _ = _step([(50, 60), (56, 67)], [[(a, 5.0)], [((56, 68), 3.0)]])
    assert st == [1, 1]                                            # 36 + 64 = 100
    out, st, _, _ = _step([(50, 60), (55, 67)], [[(a, 5.0)], [((55, 68), 3.0)]])
    assert st == [1, -1]                                           # 25 + 64 < 100


def test_a_contested_target_keeps_its_velocity():
    # alone: v' = p' - p
    out, st, nxt, new = _step([(50, 60)], [[((50, 63), 1.0)]], v=[(0, 2)])
    assert new == [(0, 3, 0)] and nxt == [(50, 66)]
    # another target's PREDICTION within d of the pick (9 columns): contested, v stays (0, 2); the other is uncontested
    out, st, nxt, new = _step([(50, 60), (50, 70)], [[((50, 63), 1.0)], [((50, 75), 1.0)]], v=[(0, 2), (0, 2)])
    assert st == [1, 1] and new == [(0, 2, 0), (0, 5, 0)] and nxt == [(50, 65), (50, 80)]
    # ... and exactly d away it is not
    out, st, nxt, new = _step([(50, 60), (50, 71)], [[((50, 63), 1.0)], [((50, 76), 1.0)]], v=[(0, 2), (0, 2)])
    assert new[0] == (0, 3, 0)
    # the other target being held does not matter: its prediction is what counts
    out, st, nxt, new = _step([(50, 60), (50, 66)], [[((50, 63), 1.0)], []], v=[(0, 2), (0, 0)])
    assert st == [1, -1] and new[0] == (0, 2, 0)
    # an assignment resets n_held
    assert _step([(50, 60)], [[((50, 63), 1.0)]], n_held=[5])[3] == [(0, 3, 0)]


@pytest.mark.parametrize("coast", [0, 1, 3])
def test_coasting(coast):
    """A target with v = (0, 7) whose windows stay empty: every held step files the prediction; the velocity survives while
    n_held' < coast — coast = 0 and 1 are the same walk, one step along v."""
    pos, v, nh = (50, 71), (0, 7), 0
    seen = []
    for _ in range(6):
        out, st, nxt, new = _step([pos], [[]], v=[v], n_held=[nh], coast=coast)
        assert st == [-1]
        pos, v, nh = out[0], new[0][:2], new[0][2]
        assert nxt == [(pos[0] + v[0], pos[1] + v[1])]
        seen.append(pos[1])
    moves = max(coast, 1)
    assert seen == [71 + 7 * min(s, moves) for s in range(1, 7)] and nh == 6 and v == (0, 0)
    # n_held stays at the top of int32
    assert _step([(5, 5)], [[]], n_held=[2**31 - 1])[3] == [(0, 0, 2**31 - 1)]


def test_clamping_at_the_frame_edge():
    # the prediction is clamped before the distances are taken and before a held target files it
    out, st, nxt, new = _step([(3, 138)], [[]], v=[(-7, 7)], coast=3)
    assert out == [(1, 140)] and new == [(-7, 7, 1)] and nxt == [(1, 140)]
    # D is measured from the clamped prediction (1, 140): (4, 139) at 10 beats (1, 144) at 16; from the unclamped (-4, 145) it would lose
    out, st, _, _ = _step([(3, 138)], [[((1, 144), 1.0), ((4, 139), 0.9)]], v=[(-7, 7)])
    assert (out, st) == ([(4, 139)], [2])
    # sums beyond int32 are formed without overflow
    big = 2**31 - 1
    out, st, nxt, new = _step([(big, -big - 1)], [[]], v=[(big, -big - 1)])
    assert out == [(100, 1)]


def test_distance_saturates():
    assert mr.dist2(0, 0, 65535, 0) == 65535 ** 2 and mr.dist2(0, 0, 65536, 0) == mr.FAR and mr.dist2(0, -65536, 0, 0) == mr.FAR
    assert mr.dist2(65535, 65535, 0, 0) == mr.FAR and mr.dist2(2**31 - 1, 0, -2**31, 0) == mr.FAR       # 2 * 65535^2 > 2^32 - 1
    assert mr.dist2(46341, 46340, 0, 0) == 46341 ** 2 + 46340 ** 2 < mr.FAR
    # two entries at FAR tie: the smaller q; a FAR entry is still a head and is taken
    out, st, _, _ = _step([(50, 60)], [[((70000, 60), 0.9), ((50, 70000), 1.0)]], rho=0.0)
    assert (out, st) == ([(70000, 60)], [1])
    # between targets whose heads are both at FAR the larger value wins
    out, st, _, _ = _step([(50, 60), (50, 90)], [[((70000, 60), 0.9)], [((70003, 60), 1.0)]])
    assert st == [-1, 1]


# ---- the host function against the restatement ----
def _host(prev, mstate, ij, peak, count, hw, d, rho, m, coast):
    G, T, k = peak.shape
    out = np.full((G, T, 2), 777, np.int32)
    state = np.full((G, T), 777, np.int32)
    nxt = np.full((G, T, 2), 777, np.int32)
    new = mstate.copy()
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = pt.lib().pdog_assign_motion_host(G, T, k, d, rho, m, coast, hw[0], hw[1], P(prev), P(new), P(ij), P(peak), P(count), P(out), P(state), P(nxt))
    return rc, out, state, nxt, new


def random_groups(rng, G, T, k, grid):
    """test_exclusive_cpu.random_groups' recipe — lattice positions, a handful of values with -inf, NaN and both zeros, unsorted,
    counts 0 ... k + 1 — plus velocities in -3 ... 3 and n_held in 0 ... 5 (word 3 is garbage: the step ignores and clears it)."""
    prev = rng.integers(0, grid, (G, T, 2)).astype(np.int32)
    ij = rng.integers(0, grid, (G, T, k, 2)).astype(np.int32)
    peak = ((rng.integers(0, 9, (G, T, k)) - 2) * 0.25).astype(np.float32)
    kind = rng.integers(0, 16, (G, T, k))
    peak[kind == 0] = NINF
    peak[kind == 1] = np.nan
    peak[kind == 2] = -0.0
    count = rng.integers(0, k + 2, (G, T)).astype(np.int32)
    mstate = np.concatenate([rng.integers(-3, 4, (G, T, 2)), rng.integers(0, 6, (G, T, 1)), rng.integers(0, 99, (G, T, 1))], axis=2).astype(np.int32)
    return prev, mstate, ij, peak, count


def test_host_function_equals_the_restatement_on_random_groups():
    rng = np.random.default_rng(20261019)
    n_groups = held = later = contested = 0
    for trial in range(700):
        T, k = (1 + trial % 32, 32 - trial % 32) if trial < 64 else (int(rng.integers(1, 33)), int(rng.integers(1, 33)))
        G, d, grid = int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 14))
        rho = [0.0, 1.0, 0.5][trial % 3] if trial % 4 == 0 else float(rng.integers(0, 1001)) / 1000.0
        m = 0.0 if trial % 3 == 0 else float(rng.integers(0, 9)) * 0.125
        coast, hw = int(rng.integers(0, 5)), (int(rng.integers(1, 2 * grid)), int(rng.integers(1, 2 * grid)))
        prev, mstate, ij, peak, count = random_groups(rng, G, T, k, grid)
        rc, out, state, nxt, new = _host(prev, mstate, ij, peak, count, hw, d, rho, m, coast)
        assert rc == _lib.PDOG_OK
        for g in range(G):
            want = mr.step(prev[g], mstate[g], ij[g], peak[g], count[g], hw, d, rho, m, coast, detail=True)
            assert np.array_equal(state[g], want[1]), (trial, g, T, k, d, rho, m, state[g], want[1])
            assert np.array_equal(out[g], want[0]) and np.array_equal(nxt[g], want[2]) and np.array_equal(new[g], want[3]), (trial, g)
            held += int((want[1] == -1).sum())
            later += int((want[1] > 1).sum())
            contested += int(want[4].sum())
        n_groups += G
    print("groups", n_groups, "held", held, "later picks", later, "contested", contested)
    assert n_groups > 1000 and held > 1000 and later > 1000 and contested > 1000      # the draw exercises what it is for


def test_host_function_refuses_bad_arguments():
    prev, mstate, ij, peak, count = random_groups(np.random.default_rng(1), 1, 2, 3, 5)
    ok = dict(G=1, T=2, k=3, d=4, rho=0.5, m=0.0, coast=2, h=9, w=9)
    L = pt.lib()
    P = lambda a: C.c_void_p(a.ctypes.data)
    out, state, nxt, new = np.full((1, 2, 2), 9, np.int32), np.full((1, 2), 9, np.int32), np.full((1, 2, 2), 9, np.int32), mstate.copy()
    for kw in (dict(G=0), dict(T=0), dict(T=33), dict(k=0), dict(k=33), dict(d=0), dict(d=-1), dict(rho=-0.01), dict(rho=1.01),
               dict(rho=float("nan")), dict(m=-1e-9), dict(m=float("nan")), dict(m=float("inf")), dict(m=1e39), dict(coast=-1), dict(h=0), dict(w=0)):
        a = dict(ok, **kw)
        assert L.pdog_assign_motion_host(a["G"], a["T"], a["k"], a["d"], a["rho"], a["m"], a["coast"], a["h"], a["w"], P(prev), P(new), P(ij),
                                         P(peak), P(count), P(out), P(state), P(nxt)) == _lib.PDOG_E_ARG, kw
        assert L.pdog_last_error() != b""
    for null in range(8):
        ptrs = [P(prev), P(new), P(ij), P(peak), P(count), P(out), P(state), P(nxt)]
        ptrs[null] = None
        assert L.pdog_assign_motion_host(1, 2, 3, 4, 0.5, 0.0, 2, 9, 9, *ptrs) == _lib.PDOG_E_ARG
    assert (out == 9).all() and (state == 9).all() and (nxt == 9).all() and np.array_equal(new, mstate)
    # the device entry points judge a null tracker before anything else: no GPU needed
    assert L.pdog_assign_motion(None, 1, 2, 3, 4, 0.5, 0.0, 2, None, None, None, None, None, None, None, None) == _lib.PDOG_E_ARG
    assert L.pdog_detect_chains_motion(None, None, 0, 0, 1, None, 1, 1, 1, 0, 0, 0, 0.5, 0.0, 2, None, None, None, None) == _lib.PDOG_E_ARG
    assert L.pdog_get_motion_counts(None, (C.c_uint64 * 2)()) == _lib.PDOG_E_ARG


# ---- the stand-alone program, plain and under the sanitizers ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_host_function_as_a_program(tmp_path, flags):
    exe = tmp_path / "motion"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "motion_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout


def test_rule_header_compiles_alone(tmp_path):
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "pdog_motion.hpp"\nint main() { return pdog::motion::admissible(0, 0, 0.f, 0.f, 0.f, 0.f) ? 1 : '
                  '(int)pdog::motion::dist2(1, 1, 1, 1) + pdog::motion::predict(5, -9, 3) - 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(tu), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


# ---- the scenes over the oracle's Float64 maps ----
@pytest.fixture(scope="module")
def walks(oracle):
    return {name: ms.walk_float64(oracle, ms.scene(name)) for name in ms.NAMES}


@pytest.mark.parametrize("name", ["through", "passing"])
def test_crossing_scenes_keep_their_identities_in_float64(walks, name):
    """What the restatement gives over the Float64 maps (printed below):
        "through"  2 steps above 3 px (steps 18 and 22, inside the merge), worst 4.0 px; states -1, 1, 2; 6 contested, 5 held
        "passing"  0 steps above 3 px, worst 0.0 px; states -1, 1, 2; 0 contested, 5 held"""
    sc = ms.scene(name)
    track, states, _, contested = walks[name]
    assert track[-1] == sc.truth[-1], (name, track[-1])                       # identities kept, exactly
    errs = ms.errors_true(track, sc.truth)
    above = ms.steps_above_true(track, sc.truth)
    print(name, "steps above 3 px:", above, [k for k, e in enumerate(errs) if e > 3], "worst:", max(errs),
          "states:", sorted({s for st in states for s in st}), "contested:", sum(map(sum, contested)), "held:", sum(s == -1 for st in states for s in st))
    assert above <= (5 if name == "through" else 0)
    d2 = es.min_assigned_distance2(track, states)
    assert d2 is not None and d2 >= sc.min_distance ** 2


def test_fast_target_in_a_small_window_in_float64(oracle, walks):
    """The restatement gives 0 steps above 3 px, worst 2.0 px (step 1, from rest); the plain chain at 11 x 11 is lost on 15 of 16
    steps and ends in the corner (1, 1)."""
    sc = ms.scene("fast")
    track, states, _, _ = walks["fast"]
    errs = ms.errors_true(track, sc.truth)
    print("fast: steps above 3 px:", ms.steps_above_true(track, sc.truth), "worst:", max(errs))
    assert ms.steps_above_true(track, sc.truth) == 0 and all(st == [1] for st in states)
    plain = ms.plain_chain_float64(oracle, sc)                                 # the premise
    print("plain chain: steps above 3 px:", ms.steps_above_true(plain, sc.truth), "final:", plain[-1])
    assert ms.steps_above_true(plain, sc.truth) >= 13


def test_vanished_target_coasts_and_stops_in_float64(walks):
    sc = ms.scene("vanish")
    track, states, resp, _ = walks["vanish"]
    assert min(r[0] for r in resp[:ms.VANISH_FROM - 1]) > 50 * sc.min_response      # the premise: 0.089 and 0.1007 against 1e-3
    assert [p[0] for p in track[ms.VANISH_FROM:]] == ms.VANISH_TAIL
    assert [st[0] for st in states] == [1] * (ms.VANISH_FROM - 1) + [-1] * (sc.nf - ms.VANISH_FROM)
    assert track[:ms.VANISH_FROM] == walks["fast"][0][:ms.VANISH_FROM]


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


def test_motion_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.MOTION_PROTOTYPES) == [
        "pdog_assign_motion", "pdog_assign_motion_host", "pdog_detect_chains_motion", "pdog_get_motion_counts"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.MOTION_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert [len(a) for _, a in protos] == [16, 17, 19, 2]
    hdr = open(HDR).read()
    assert "#define PDOG_MOTION_MAX_TARGETS 32" in hdr and _lib.MOTION_MAX_TARGETS == mr.MAX_TARGETS == 32
    assert pt.lib().pdog_abi_version() == 1          # an addition: the version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pawsome_motion.h" in mk and "$(O)/pawsome_motion.o" in mk
    # the kernel and the host function share the rule's header, which takes blocking and the round's order from the exclusive one
    for unit in ("dog_motion.hpp", "pdog_math.cpp"):
        assert '#include "pdog_motion.hpp"' in open(os.path.join(CSRC, unit)).read(), unit
    assert '#include "pdog_exclusive.hpp"' in open(os.path.join(CSRC, "pdog_motion.hpp")).read()
    # the earlier tables hold nothing of this header's
    assert not set(_lib.MOTION_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.PEAKS_PROTOTYPES) | set(_lib.EXCLUSIVE_PROTOTYPES))
    par = inspect.signature(pt.track_video).parameters
    assert list(par)[-5:] == ["motion", "coast", "min_response", "exclusive", "min_ratio"]
    assert par["motion"].default is False and par["coast"].default is None and par["min_response"].default is None
    assert list(inspect.signature(pt.BatchTracker.assign_motion).parameters)[1:] == [
        "prev", "mstate", "ij", "peak", "count", "min_distance", "min_ratio", "min_response", "coast"]
    sig = inspect.signature(pt.BatchTracker.detect_chains_motion).parameters
    assert list(sig)[1:] == ["frames", "frame_table", "starts", "k", "min_distance", "min_ratio", "min_response", "coast", "first", "mstate"]
    assert (sig["min_ratio"].default, sig["min_response"].default, sig["coast"].default, sig["first"].default) == (0.5, 0.0, 8, 0)
    assert sig["k"].default is None and sig["mstate"].default is None


def test_headers_compile_alone(tmp_path):
    for hdr in (HDR, os.path.join(ROOT, "include", "pawsome_exclusive.h")):
        for cc, flags in (("gcc", ["-x", "c", "-std=c99", "-Wextra"]), ("g++", ["-x", "c++"])):
            subprocess.check_call([cc] + flags + ["-fsyntax-only", "-Wall", "-Werror", hdr])


def test_python_arguments_are_checked():
    assert _args.motion_args(2, None, None, 0.5, 0.0, 8) == (0, 0, 0.5, 0.0, 8) and _args.motion_args(32, 4, 7, 1, 1, 0) == (4, 7, 1.0, 1.0, 0)
    for exc, a in ((ValueError, (0, None, None, 0.5, 0.0, 8)), (ValueError, (33, None, None, 0.5, 0.0, 8)), (ValueError, (2, 33, None, 0.5, 0.0, 8)),
                   (TypeError, (2, 2.0, None, 0.5, 0.0, 8)), (ValueError, (2, 2, 0, 0.5, 0.0, 8)), (ValueError, (2, 2, None, 1.1, 0.0, 8)),
                   (TypeError, (2, 2, None, None, 0.0, 8)), (ValueError, (2, 2, None, 0.5, -1e-9, 8)), (ValueError, (2, 2, None, 0.5, float("nan"), 8)),
                   (ValueError, (2, 2, None, 0.5, float("inf"), 8)), (ValueError, (2, 2, None, 0.5, 1e39, 8)), (TypeError, (2, 2, None, 0.5, "0", 8)),
                   (TypeError, (2, 2, None, 0.5, True, 8)), (TypeError, (2, 2, None, 0.5, None, 8)), (ValueError, (2, 2, None, 0.5, 0.0, -1)),
                   (TypeError, (2, 2, None, 0.5, 0.0, 2.0)), (TypeError, (2, 2, None, 0.5, 0.0, True)), (TypeError, (2, 2, None, 0.5, 0.0, None)),
                   (ValueError, (2, 2, None, 0.5, 0.0, 2**31))):
        with pytest.raises(exc) as e:
            _args.motion_args(*a)
        assert type(e.value) is exc, a
    import torch
    frames = torch.zeros((2, 40, 40), dtype=torch.uint8)
    for kw, exc, match in ((dict(coast=3), ValueError, "coast"), (dict(min_response=0.1), ValueError, "min_response"),
                           (dict(exclusive=True, coast=3), ValueError, "coast"), (dict(motion=True, exclusive=True), ValueError, "exclusive"),
                           (dict(motion=1), TypeError, "motion"), (dict(motion=True, coast=-1), ValueError, "coast"),
                           (dict(motion=True, coast=1.5), TypeError, "coast"), (dict(motion=True, min_response=-1.0), ValueError, "min_response"),
                           (dict(motion=True, min_ratio=1.5), ValueError, "min_ratio"), (dict(motion=True, min_distance=0), ValueError, "min_distance"),
                           (dict(motion=True, start_locations=[None] * 33), ValueError, "n_targets"),
                           # what held without the keyword holds with it
                           (dict(min_ratio=0.5), ValueError, "min_ratio"), (dict(min_distance=5), ValueError, "min_distance"),
                           (dict(exclusive=1), TypeError, "exclusive")):
        with pytest.raises(exc, match=match):                      # judged before anything touches the device
            pt.track_video(frames, 24, **kw)
