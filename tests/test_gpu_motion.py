"""The motion step and walk on the GPU (include/pawsome_motion.h).

Every comparison of positions, states, next guesses and mstate is exact.  assign_motion is held to tests/motion_restatement.py
on seeded random groups, in both forms of the kernel (lists read from global memory, lists staged in LDS); detect_chains_motion
is replayed step by step — detect_peaks at the replay's own predictions, the restatement on its result — on the four scenes of
tests/motion_scenes.py, which also have to come out as the issue of this feature asks: identities kept where two discs cross, a
fast disc followed in a window a plain chain loses it in, a vanished disc coasted after and then left alone.  The whole file
fails on a library without the symbols."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusive_scenes as es  # noqa: E402
import motion_restatement as mr  # noqa: E402
import motion_scenes as ms  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_detect_chains_motion")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def trackers(pt):
    """One tracker per window size the scenes use (21, 41, 11), made on demand."""
    made = {}

    def get(ws):
        if ws not in made:
            made[ws] = pt.BatchTracker(ms.H, ms.W, ms.TW, (ws, ws), True, ms.BKGD)
        return made[ws]
    yield get
    for t in made.values():
        t.close()


# ---- assign_motion, bit for bit ----
def _random_groups(rng, G, T, k, grid):
    """tests/test_motion_cpu.py's recipe: lattice positions (blocking and equal distances are common), a handful of values with
    -inf, NaN and both zeros, unsorted, counts 0 ... k + 1, velocities in -3 ... 3, n_held in 0 ... 5, garbage in word 3."""
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


@pytest.fixture(scope="module")
def kernel_cases():
    """64 calls, 208 groups: T = 1 ... 32 with k = 32 ... 1 once each (3 groups a call), then 32 random shapes; one call in
    eight with positions and velocities at the ends of int32.  The restatement's answers are computed once."""
    rng = np.random.default_rng(20261019)
    cases = []
    for c in range(64):
        T, k = (1 + c, 32 - c) if c < 32 else (int(rng.integers(1, 33)), int(rng.integers(1, 33)))
        G = 3 if c < 32 else 2 + c % 4
        d, grid, coast = int(rng.integers(1, 7)), int(rng.integers(2, 14)), int(rng.integers(0, 5))
        rho = [0.0, 1.0, 0.5][c % 3] if c % 4 == 0 else float(rng.integers(0, 1001)) / 1000.0
        m = 0.0 if c % 3 == 0 else float(rng.integers(0, 9)) * 0.125
        arrays = _random_groups(rng, G, T, k, grid)
        if c % 8 == 7:
            ext = lambda shape: np.where(rng.integers(0, 2, shape) == 1, 2**31 - 1 - rng.integers(0, 3, shape), -2**31 + rng.integers(0, 3, shape))
            prev, mstate, ij, peak, count = arrays
            prev = np.where(rng.integers(0, 2, prev.shape) == 1, ext(prev.shape), prev).astype(np.int32)
            ij = np.where(rng.integers(0, 4, ij.shape) == 0, ext(ij.shape), ij + 65536 * rng.integers(0, 2, ij.shape)).astype(np.int32)
            mstate[..., :2] = np.where(rng.integers(0, 2, (G, T, 2)) == 1, ext((G, T, 2)), mstate[..., :2])
            mstate[..., 2] = np.where(rng.integers(0, 4, (G, T)) == 0, 2**31 - 1, mstate[..., 2])
            arrays = (prev, mstate.astype(np.int32), ij, peak, count)
        want = mr.step_groups(*arrays, (ms.H, ms.W), d, rho, m, coast)
        cases.append((arrays, (d, rho, m, coast), want))
    assert sum(len(a[0]) for a, _, _ in cases) >= 200
    assert sorted({a[3].shape[1] for a, _, _ in cases[:32]}) == sorted({a[3].shape[2] for a, _, _ in cases[:32]}) == list(range(1, 33))
    return cases


@pytest.mark.parametrize("lds", [False, True], ids=["global", "lds"])
def test_kernel_equals_the_restatement(trackers, kernel_cases, lds):
    bt = trackers(21)
    bt.set_tuning("motion_lds", lds)
    try:
        seen = set()
        for (prev, mstate, ij, peak, count), (d, rho, m, coast), want in kernel_cases:
            d_ms = _cuda(mstate)
            out, state, nxt = bt.assign_motion(_cuda(prev), d_ms, _cuda(ij), _cuda(peak), _cuda(count), d, rho, m, coast)
            bt.sync()
            got = [x.cpu().numpy() for x in (out, state, nxt, d_ms)]
            shape = (peak.shape, d, rho, m, coast)
            assert np.array_equal(got[1], want[1]), (shape, got[1], want[1])
            for a, b, what in zip(got, want, ("positions", "states", "next guesses", "mstate")):
                assert np.array_equal(a, b), (what, shape)
            seen |= set(want[1].ravel().tolist())
        assert -1 in seen and max(seen) >= 8, seen         # holds and late picks occur
    finally:
        bt.set_tuning("motion_lds", False)


# ---- detect_chains_motion, replayed step by step ----
def _picks(bt, d_frames, guess, fi, k, md):
    """detect_peaks for the G x T windows at guess [G, T, 2] on frames fi [G]: host copies shaped [G, T, ...]."""
    G, T = guess.shape[:2]
    ij, peak, count = bt.detect_peaks(d_frames, _cuda(guess.reshape(-1, 2)), k, md, _cuda(np.repeat(fi, T).astype(np.int32)))
    bt.sync()
    return ij.view(G, T, k, 2).cpu().numpy(), peak.view(G, T, k).cpu().numpy(), count.view(G, T).cpu().numpy()


def _replay(bt, d_frames, table, starts, out, state, first, k, md, rho, m, coast, mstate0=None):
    """Walks the restatement beside the library's outputs.  Returns (final positions, final mstate, states seen, pick 1's
    responses by step)."""
    G, T = starts.shape[:2]
    hw = (bt.frame_h, bt.frame_w)
    lens = [int((row >= 0).sum()) for row in table]
    pos = starts.astype(np.int32).copy()
    mst = np.zeros((G, T, 4), np.int32) if mstate0 is None else mstate0.copy()
    guess = np.array([[(mr.clamp(int(pos[g, t, 0]) + int(mst[g, t, 0]), hw[0]), mr.clamp(int(pos[g, t, 1]) + int(mst[g, t, 1]), hw[1]))
                       for t in range(T)] for g in range(G)], np.int32)
    for g in range(G):
        assert (out[g, :, lens[g]:] == 0).all() and (state[g, :, lens[g]:] == 0).all(), g      # an ended row stores nothing
        if first and lens[g] >= 1:
            assert np.array_equal(out[g, :, 0], starts[g]) and (state[g, :, 0] == 0).all()
    seen, resp = set(), []
    for s in range(first, table.shape[1]):
        live = [g for g in range(G) if lens[g] > s]
        if not live:
            break
        fi = np.array([table[g, min(s, lens[g] - 1)] if lens[g] else 0 for g in range(G)], np.int32)
        ij, peak, count = _picks(bt, d_frames, guess, fi, k, md)
        resp.append(peak[:, :, 0].copy())
        for g in live:
            p2, st, nxt, new = mr.step(pos[g], mst[g], ij[g], peak[g], count[g], hw, md, rho, m, coast)
            assert np.array_equal(state[g, :, s], st), (first, s, g, state[g, :, s], st)
            assert np.array_equal(out[g, :, s], p2), (first, s, g, out[g, :, s], p2)
            pos[g], mst[g], guess[g] = p2, new, nxt
            seen |= set(st.tolist())
    return pos, mst, seen, resp


def _walk_scene(bt, sc, m=None):
    d_frames = _cuda(sc.frames)
    table = np.arange(sc.nf, dtype=np.int32)[None]
    starts = np.array([sc.starts], np.int32)
    m = sc.min_response if m is None else m
    out, state, mstate = bt.detect_chains_motion(d_frames, table, _cuda(starts), sc.k, sc.min_distance, sc.ratio, m, sc.coast, first=1)
    bt.sync()
    out, state, mstate = out.cpu().numpy(), state.cpu().numpy(), mstate.cpu().numpy()
    pos, mst, seen, resp = _replay(bt, d_frames, table, starts, out, state, 1, sc.k, sc.min_distance, sc.ratio, m, sc.coast)
    assert np.array_equal(mstate, mst) and np.array_equal(out[:, :, -1], pos)
    track = [[tuple(int(v) for v in out[0, t, f]) for t in range(len(sc.starts))] for f in range(sc.nf)]
    states = [[int(state[0, t, f]) for t in range(len(sc.starts))] for f in range(1, sc.nf)]
    return track, states, resp, d_frames


@pytest.mark.parametrize("name", ["through", "passing"])
def test_crossing_scenes_keep_their_identities(trackers, name):
    sc = ms.scene(name)
    track, states, _, _ = _walk_scene(trackers(sc.ws[0]), sc)
    above = ms.steps_above_true(track, sc.truth)
    print(name, "steps above 3 px against the true labelling:", above, "worst:", max(ms.errors_true(track, sc.truth)), "final:", track[-1],
          "states:", sorted({s for st in states for s in st}))
    assert max(ms.errors_true(track, sc.truth)[-1:]) <= 1, (name, track[-1])          # identities kept: each target on ITS disc
    assert above <= es.GPU_STEPS_ABOVE_3PX, (name, above)                               # (a lost identity costs 18)
    d2 = es.min_assigned_distance2(track, states)
    assert d2 is not None and d2 >= sc.min_distance ** 2


def test_fast_target_in_a_small_window(trackers):
    sc = ms.scene("fast")
    bt = trackers(sc.ws[0])
    track, states, _, d_frames = _walk_scene(bt, sc)
    above = ms.steps_above_true(track, sc.truth)
    print("fast: steps above 3 px:", above, "worst:", max(ms.errors_true(track, sc.truth)), "final:", track[-1])
    assert above <= 1 and all(st == [1] for st in states)
    # the plain chain at the same window loses the target
    plain = bt.detect_chains_indexed(d_frames, np.arange(sc.nf, dtype=np.int32)[None], _cuda(np.array(sc.starts, np.int32)), first=1)
    bt.sync()
    plain = [[tuple(int(v) for v in p)] for p in plain.cpu().numpy()[0]]
    print("plain chain: steps above 3 px:", ms.steps_above_true(plain, sc.truth), "final:", plain[-1])
    assert ms.steps_above_true(plain, sc.truth) >= 13


@pytest.mark.parametrize("m", [ms.VANISH_MIN_RESPONSE, 0.0])
def test_vanished_target_coasts_and_stops(trackers, m):
    """With min_response 0 too: the flat window's FP32 response is exactly 0, which does not exceed 0."""
    sc = ms.scene("vanish")
    track, states, resp, _ = _walk_scene(trackers(sc.ws[0]), sc, m=m)
    assert min(float(r[0, 0]) for r in resp[:ms.VANISH_FROM - 1]) > 50 * ms.VANISH_MIN_RESPONSE        # the premise
    assert all(float(r[0, 0]) == 0.0 for r in resp[ms.VANISH_FROM - 1:])
    assert [p[0] for p in track[ms.VANISH_FROM:]] == ms.VANISH_TAIL
    assert [st[0] for st in states] == [1] * (ms.VANISH_FROM - 1) + [-1] * (sc.nf - ms.VANISH_FROM)


# ---- static targets, several groups, split walks, repeat calls ----
def test_static_discs_walk_their_indexed_chains(trackers):
    bt = trackers(21)
    centres = [(40, 40), (60, 100)]
    frames = np.stack([es.draw((ms.H, ms.W), [(c, 0) for c in centres])] * 6)
    frames[1::2] += 1                                                   # (the frames differ, the discs stay)
    d_frames = _cuda(frames)
    table = np.arange(6, dtype=np.int32)
    starts = np.array([(38, 41), (62, 98)], np.int32)                   # two pixels off: step 0 moves, then nothing does
    want = bt.detect_chains_indexed(d_frames, np.tile(table, (2, 1)), _cuda(starts))
    out, state, mstate = bt.detect_chains_motion(d_frames, table[None], _cuda(starts[None]), coast=0)
    bt.sync()
    # step 0 leaves v = (2, -1) and (-2, 2): step 1's windows are centred two pixels past the discs, which they still hold
    assert np.array_equal(out.cpu().numpy()[0], want.cpu().numpy()) and (state.cpu().numpy() == 1).all()
    assert np.array_equal(out.cpu().numpy()[0, :, -1], np.array(centres)) and (mstate.cpu().numpy() == 0).all()


@pytest.fixture(scope="module")
def stack():
    """"through" and "passing" in ONE stack of 82 frames: clip c's frame f is stack frame 41 * c + f."""
    return _cuda(np.concatenate([es.scene("through").frames, es.scene("passing").frames]))


@pytest.mark.parametrize("first", [0, 1])
def test_groups_with_rows_of_unequal_length(trackers, stack, first):
    """Three groups of two targets around the crossing: group 0's row drops a frame, group 1 ("passing") runs on, group 2 ends
    after five steps; a group that has ended neither stores anything nor changes what the others do."""
    bt = trackers(41)
    rows = [[10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 22], [10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21], [14, 15, 16, 17, 18] + [-1] * 7]
    clips = (0, 1, 0)
    table = np.array([[41 * c + f if f >= 0 else -1 for f in row] for c, row in zip(clips, rows)], np.int32)
    truth = lambda c, f: (es.scene("through") if c == 0 else es.scene("passing")).truth[f]
    starts = np.array([truth(c, row[0]) for c, row in zip(clips, rows)], np.int32)
    k, md, rho, m, coast = 4, es.MIN_DISTANCE, 0.5, 0.0, 2
    out, state, mstate = bt.detect_chains_motion(stack, table, _cuda(starts), k, md, rho, m, coast, first)
    bt.sync()
    out, state, mstate = out.cpu().numpy(), state.cpu().numpy(), mstate.cpu().numpy()
    _, mst, seen, _ = _replay(bt, stack, table, starts, out, state, first, k, md, rho, m, coast)
    assert np.array_equal(mstate, mst) and 1 in seen
    out2, state2, mstate2 = bt.detect_chains_motion(stack, table[:2], _cuda(starts[:2]), k, md, rho, m, coast, first)
    bt.sync()
    assert np.array_equal(out2.cpu().numpy(), out[:2]) and np.array_equal(state2.cpu().numpy(), state[:2]) and np.array_equal(mstate2.cpu().numpy(), mstate[:2])
    # a group without a step leaves the mstate it was given
    given = _cuda(np.full((3, 2, 4), 5, np.int32))
    table0 = table.copy()
    table0[2] = -1
    bt.detect_chains_motion(stack, table0, _cuda(starts), k, md, rho, m, coast, first, mstate=given)
    bt.sync()
    assert (given.cpu().numpy()[2] == 5).all() and (given.cpu().numpy()[:2, :, 3] == 0).all()


@pytest.mark.parametrize("first", [0, 1])
def test_a_walk_split_into_two_calls(trackers, first):
    """Frames 0 ... 24 of "through" in one call, and in two: the second starts from the first's last positions and mstate."""
    sc = ms.scene("through")
    bt = trackers(sc.ws[0])
    d_frames = _cuda(sc.frames)
    table = np.arange(25, dtype=np.int32)[None]
    starts = _cuda(np.array([sc.starts], np.int32))
    args = (sc.k, sc.min_distance, sc.ratio, 0.0, 3)
    one = bt.detect_chains_motion(d_frames, table, starts, *args, first=first)
    a = bt.detect_chains_motion(d_frames, table[:, :14], starts, *args, first=first)
    assert int(a[2].abs().sum()) > 0                                          # the targets move: the state matters
    b = bt.detect_chains_motion(d_frames, table[:, 14:], a[0][:, :, -1].contiguous(), *args, first=0, mstate=a[2])
    bt.sync()
    import torch
    assert torch.equal(torch.cat([a[0], b[0]], 2), one[0]) and torch.equal(torch.cat([a[1], b[1]], 2), one[1]) and torch.equal(b[2], one[2])
    assert b[2] is a[2]                                                       # updated in place


def test_a_repeated_call_allocates_nothing(pt, trackers, stack):
    import torch
    bt = trackers(41)
    table = np.array([[41 * c + f for f in range(15, 25)] for c in (0, 1, 0)], np.int32)
    starts = _cuda(np.array([es.scene("through").truth[15] * 4, es.scene("passing").truth[15] * 4, es.scene("through").truth[15] * 4], np.int32).reshape(3, 8, 2))
    one = bt.detect_chains_motion(stack, table, starts, first=1)
    bt.sync()
    torch.cuda.synchronize()
    counts = bt.motion_counts()
    L, P = pt.lib(), lambda t: C.c_void_p(t.data_ptr())
    out, state, mstate = torch.zeros_like(one[0]), torch.zeros_like(one[1]), torch.zeros_like(one[2])
    free = torch.cuda.mem_get_info()[0]
    for d_ms in (P(mstate), None):
        assert L.pdog_detect_chains_motion(bt._h, P(stack), stack.stride(0), stack.stride(1), stack.shape[0], C.c_void_p(table.ctypes.data), 10, 3, 8, 1,
                                           0, 0, 0.5, 0.0, 8, P(starts), P(out), P(state), d_ms) == 0
    bt.sync()
    after = bt.motion_counts()
    assert after[1] == counts[1] and after[0] == counts[0] + 18         # no workspace grew; twice nine steps
    assert torch.cuda.mem_get_info()[0] == free                          # nor did anything else in the library allocate
    assert torch.equal(out, one[0]) and torch.equal(state, one[1]) and torch.equal(mstate, one[2])


def test_bad_arguments_launch_nothing(pt, trackers, stack):
    import torch
    from pawsometracker_jl_amd import _lib
    bt = trackers(41)
    L, P = pt.lib(), lambda t: C.c_void_p(t.data_ptr())
    G, T, k, ns = 2, 3, 4, 5
    table = np.array([[0, 1, 2, 3, 4], [41, 42, 43, -1, -1]], np.int32)
    starts = _cuda(np.full((G, T, 2), 50, np.int32))
    out = torch.zeros((G, T, ns, 2), dtype=torch.int32, device="cuda")
    state = torch.zeros((G, T, ns), dtype=torch.int32, device="cuda")
    mstate = torch.full((G, T, 4), 3, dtype=torch.int32, device="cuda")
    ok = dict(t=bt._h, f=P(stack), fs=stack.stride(0), rs=stack.stride(1), nf=stack.shape[0], tab=table, ns=ns, G=G, T=T, first=0, k=k, md=0,
              rho=0.5, m=0.0, coast=2, st=P(starts), o=P(out), s=P(state), ms=P(mstate))

    def walk(**kw):
        a = dict(ok, **kw)
        tab = None if a["tab"] is None else C.c_void_p(np.ascontiguousarray(a["tab"], np.int32).ctypes.data)
        return L.pdog_detect_chains_motion(a["t"], a["f"], a["fs"], a["rs"], a["nf"], tab, a["ns"], a["G"], a["T"], a["first"], a["k"], a["md"],
                                           a["rho"], a["m"], a["coast"], a["st"], a["o"], a["s"], a["ms"])

    bt.sync()
    before = (bt.motion_counts(), bt.peaks_counts())
    bad_entry = table.copy()
    bad_entry[0, 2] = stack.shape[0]
    for kw in (dict(t=None), dict(f=None), dict(tab=None), dict(st=None), dict(o=None), dict(s=None), dict(T=0), dict(T=33), dict(k=33),
               dict(rho=-0.1), dict(rho=float("nan")), dict(m=-0.5), dict(m=float("nan")), dict(m=float("inf")), dict(coast=-1), dict(G=0),
               dict(ns=0), dict(nf=0), dict(first=2), dict(rs=ms.W - 1), dict(fs=-1), dict(tab=bad_entry)):
        assert walk(**kw) == _lib.PDOG_E_ARG, kw
        assert L.pdog_last_error() != b""
    prev, ij = torch.zeros((G, T, 2), dtype=torch.int32, device="cuda"), torch.zeros((G, T, k, 2), dtype=torch.int32, device="cuda")
    peak, count = torch.ones((G, T, k), device="cuda"), torch.ones((G, T), dtype=torch.int32, device="cuda")
    o2, s2, n2 = torch.zeros_like(prev), torch.zeros((G, T), dtype=torch.int32, device="cuda"), torch.zeros_like(prev)
    aok = [bt._h, G, T, k, 0, 0.5, 0.0, 2, P(prev), P(mstate), P(ij), P(peak), P(count), P(o2), P(s2), P(n2)]
    for pos, v in ((0, None), (1, 0), (2, 0), (2, 33), (3, 0), (3, 33), (5, -0.5), (5, float("nan")), (6, -1.0), (6, float("nan")), (6, float("inf")),
                   (7, -1), (8, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None)):
        a = list(aok)
        a[pos] = v
        assert L.pdog_assign_motion(*a) == _lib.PDOG_E_ARG, (pos, v)
    bt.sync()                                                    # clean: nothing was launched
    assert (bt.motion_counts(), bt.peaks_counts()) == before
    assert int(out.abs().sum()) == 0 and int(state.abs().sum()) == 0 and int(s2.abs().sum()) == 0 and bool((mstate == 3).all())
    for exc, call in ((ValueError, lambda: bt.detect_chains_motion(stack, table, starts, coast=-1)),
                      (TypeError, lambda: bt.detect_chains_motion(stack, table, starts, coast=1.0)),
                      (ValueError, lambda: bt.detect_chains_motion(stack, table, starts, min_response=-1)),
                      (ValueError, lambda: bt.detect_chains_motion(stack, table, starts, first=2)),
                      (ValueError, lambda: bt.detect_chains_motion(stack, table, starts, mstate=mstate[:1])),
                      (TypeError, lambda: bt.detect_chains_motion(stack, table, starts, mstate=mstate.cpu())),
                      (TypeError, lambda: bt.detect_chains_motion(stack, table, starts.cpu())),
                      (TypeError, lambda: bt.assign_motion(prev, mstate.float(), ij, peak, count)),
                      (ValueError, lambda: bt.assign_motion(prev, mstate[:, :, :3].contiguous(), ij, peak, count)),
                      (ValueError, lambda: bt.assign_motion(prev, mstate, ij, peak, count, min_response=float("nan")))):
        with pytest.raises(exc):
            call()
    bt.sync()
    assert (bt.motion_counts(), bt.peaks_counts()) == before
    assert walk() == _lib.PDOG_OK                                # and the tracker works afterwards
    bt.sync()
    assert bt.motion_counts()[0] == before[0][0] + 5 and int(state[0].abs().sum()) > 0 and int(state[1, :, 3:].abs().sum()) == 0


# ---- end to end ----
def test_track_video_with_a_motion_model(pt, trackers):
    sc = ms.scene("through")
    d_frames = _cuda(sc.frames)
    args = dict(rate=24, start=0, stop=sc.nf / 24, fps=24, target_width=ms.TW, window_size=sc.ws[0], start_locations=[("ij", c) for c in sc.starts])
    ts, idx, state = pt.track_video(d_frames, motion=True, min_ratio=sc.ratio, min_distance=sc.min_distance, coast=sc.coast,
                                    min_response=sc.min_response, **args)
    assert idx.shape == (2, sc.nf, 2) and state.shape == (2, sc.nf) and len(ts) == sc.nf
    # the walk's positions and states: track_video bootstraps on frame 0 at the given locations (the discs' centres, where the
    # functor stays) and walks the rest as one group
    bt = trackers(sc.ws[0])
    out, st, _ = bt.detect_chains_motion(d_frames, np.arange(sc.nf, dtype=np.int32)[None], idx[:, 0].contiguous().unsqueeze(0), None, sc.min_distance,
                                         sc.ratio, sc.min_response, sc.coast, first=1)
    bt.sync()
    import torch
    assert torch.equal(idx, out[0]) and torch.equal(state, st[0]) and bool((state[:, 0] == 0).all())
    track = [[tuple(int(v) for v in idx[t, f].cpu().numpy()) for t in range(2)] for f in range(sc.nf)]
    assert track[0] == sc.starts and max(ms.errors_true(track, sc.truth)[-1:]) <= 1          # identities kept
    ts2, plain = pt.track_video(d_frames, **args)                                             # without the keyword: as before
    assert np.array_equal(ts, ts2) and plain.shape == idx.shape
    # subpixel and the overlay work on the positions as before
    seen = []
    res = pt.track_video(d_frames, motion=True, subpixel=True, diagnostic=lambda k0, ov: seen.append((k0, int(ov.shape[0]))), min_distance=sc.min_distance, **args)
    assert len(res) == 4 and torch.equal(res[1], idx) and torch.equal(res[3], state)
    assert res[2].shape == (2, sc.nf, 2) and sum(n for _, n in seen) == sc.nf - 1
