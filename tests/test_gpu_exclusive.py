"""The exclusive step and walk on the GPU (include/pawsome_exclusive.h).

Every comparison of positions and states is exact.  assign_exclusive is held to tests/exclusive_restatement.py applied to the
picks detect_peaks returned IN THE SAME TEST; detect_chains_exclusive is replayed step by step — detect_peaks on the walk's own
previous positions, the restatement on its result —; one target per group equals detect_chains_indexed, two far-apart targets
their independent chains; and the two scenes of tests/exclusive_scenes.py run end to end through track_video: independent
chains collapse onto one disc, the exclusive walk keeps one target on each.  The whole file fails on a library without the
symbols."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusive_restatement as er  # noqa: E402
import exclusive_scenes as es  # noqa: E402
import peaks_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu
WS = 41                      # one window for the stacked clips: "passing"'s


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_detect_chains_exclusive")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def stack():
    """Three clips in ONE stack of 123 frames: "through", "passing", and "through" under +-3 levels of noise (many weak local
    maxima: long pick lists).  clip c's frame f is stack frame 41 * c + f."""
    a, b = es.scene("through").frames, es.scene("passing").frames
    noise = np.random.default_rng(5).integers(-3, 4, a.shape)
    c = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    frames = np.concatenate([a, b, c])
    return frames, _cuda(frames)


@pytest.fixture(scope="module")
def bt(pt):
    t = pt.BatchTracker(es.H, es.W, es.TW, (WS, WS), True, es.BKGD)
    yield t
    t.close()


def _targets(clip, frame, T, seed):
    """T positions for a group looking at `frame` of `clip`: the two discs' centres, then jittered copies of them — windows that
    see the same blobs, so that picks are contested, later picks taken and targets held."""
    sc = es.scene("passing" if clip == 1 else "through")
    rng = np.random.default_rng(seed)
    base = [sc.truth[frame][t % 2] for t in range(T)]
    jit = rng.integers(-12, 13, (T, 2))
    jit[:2] = 0
    return (np.array(base) + jit).astype(np.int32)[:T]


def _picks(bt, d_frames, prev, fi, k, md):
    """detect_peaks for the G x T windows at prev [G, T, 2] on frames fi [G]: host copies shaped [G, T, ...] and the device ones."""
    G, T = prev.shape[:2]
    d_prev = _cuda(prev.reshape(-1, 2))
    ij, peak, count = bt.detect_peaks(d_frames, d_prev, k, md, _cuda(np.repeat(fi, T).astype(np.int32)))
    dev = (d_prev.view(G, T, 2), ij.view(G, T, k, 2), peak.view(G, T, k), count.view(G, T))
    bt.sync()
    return [x.cpu().numpy() for x in dev], dev


# ---- assign_exclusive, bit for bit ----
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 4, 32])
def test_assign_equals_the_restatement(bt, stack, G, T):
    """k = 1, 4 and 32 (the last two also with min_distance 4 and ratio 0: long lists, much blocking) on frames around the
    crossing, where both discs lie in every window."""
    _, d_frames = stack
    seen = set()
    for k, md, rho in ((1, None, 0.5), (4, None, 0.5), (4, 4, 0.0), (32, None, 0.5), (32, 4, 0.0), (32, 4, 1.0)):
        frame = 17 + (k + T) % 4
        prev = np.stack([_targets(c, frame, T, 100 * c + T + k) for c in (2, 1, 0)[:G]])
        fi = np.array([41 * c + frame for c in (2, 1, 0)[:G]], np.int32)
        host, dev = _picks(bt, d_frames, prev, fi, k, md)
        out, state = bt.assign_exclusive(*dev, min_distance=md, min_ratio=rho)
        bt.sync()
        d = md or pr.default_min_distance(es.TW)
        want, wstate = er.assign_groups(*host, d, rho)
        assert np.array_equal(state.cpu().numpy(), wstate), (G, T, k, md, rho, state.cpu().numpy(), wstate)
        assert np.array_equal(out.cpu().numpy(), want), (G, T, k, md, rho)
        seen |= set(wstate.ravel().tolist())
        if T == 1:
            assert (wstate == 1).all() and np.array_equal(want, host[1][:, :, 0])
    if T >= 4:
        assert -1 in seen and max(seen) >= 2, seen        # the inputs exercise holds and later picks


# ---- detect_chains_exclusive, replayed step by step ----
def _replay(bt, d_frames, table, starts, out, state, first, k, md, rho):
    G, T = starts.shape[:2]
    lens = [(int((row >= 0).sum())) for row in table]
    d = md or pr.default_min_distance(bt.info().target_width)
    for g in range(G):
        assert (out[g, :, lens[g]:] == 0).all() and (state[g, :, lens[g]:] == 0).all(), g      # an ended row stores nothing
        if first and lens[g] >= 1:
            assert np.array_equal(out[g, :, 0], starts[g]) and (state[g, :, 0] == 0).all()
    seen = set()
    for s in range(first, table.shape[1]):
        live = [g for g in range(G) if lens[g] > s]
        if not live:
            break
        prev = np.stack([starts[g] if s == 0 or g not in live else out[g, :, s - 1] for g in range(G)])   # (ended: any valid guess)
        fi =np.array([table[g, min(s, lens[g] - 1)] if lens[g] else 0 for g in range(G)], np.int32)
        host, _ = _picks(bt, d_frames, np.ascontiguousarray(prev), fi, k, md)
        want, wstate = er.assign_groups(*host, d, rho)
        for g in live:
            assert np.array_equal(state[g, :, s], wstate[g]), (first, s, g, state[g, :, s], wstate[g])
            assert np.array_equal(out[g, :, s], want[g]), (first, s, g)
            seen |= set(wstate[g].tolist())
    return seen


@pytest.mark.parametrize("first", [0, 1])
def test_walk_replays_step_by_step(bt, stack, first):
    """Three groups of four targets over frames 12 ... 27 of their clips: group 0's row drops a slot (… 15, 17 …), group 1's
    repeats one (… 15, 15 …), group 2's ends after six steps."""
    _, d_frames = stack
    rows = [[12, 13, 14, 15, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26], [12, 13, 14, 15, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24],
            [14, 15, 16, 17, 18, 19] + [-1] * 8]
    table = np.array([[41 * c + f if f >= 0 else -1 for f in row] for c, row in zip((0, 1, 2), rows)], np.int32)
    starts = np.stack([_targets(c, rows[c][0], 4, 7 + c) for c in range(3)])
    k, md, rho = 4, None, 0.5
    out, state = bt.detect_chains_exclusive(d_frames, table, _cuda(starts), k, md, rho, first)
    bt.sync()
    out, state = out.cpu().numpy(), state.cpu().numpy()
    seen = _replay(bt, d_frames, table, starts, out, state, first, k, md, rho)
    assert {-1, 1, 2} <= seen, seen
    # group 2 ended early: the other groups walk as they do without it
    out2, state2 = bt.detect_chains_exclusive(d_frames, table[:2], _cuda(starts[:2]), k, md, rho, first)
    bt.sync()
    assert np.array_equal(out2.cpu().numpy(), out[:2]) and np.array_equal(state2.cpu().numpy(), state[:2])


def test_walk_on_the_headline_shape(pt):
    """Target width 25 (l = 65), 45 x 45 windows on 240 x 320 frames, the tracker pinned to its own batch kernel family (the
    benchmark's): three discs of radius 12 that meet in the middle, k and min_distance the defaults (6 and 25)."""
    nf, h, w = 14, 240, 320
    centres = lambda k: [(120, 100 + 6 * k), (120, 220 - 6 * k), (60 + 6 * k, 160)]
    frames = np.stack([es.draw((h, w), list(zip(centres(k), (0, 40, 80))), radius=12) for k in range(nf)])
    d_frames = _cuda(frames)
    t = pt.BatchTracker(h, w, 25, (45, 45), True, 128)
    try:
        assert t.info().kernel_len == 65
        t.set_variant(t.info().variant)
        table = np.arange(nf, dtype=np.int32)[None]
        starts = np.array([centres(0)], np.int32)
        out, state = t.detect_chains_exclusive(d_frames, table, _cuda(starts), first=1)
        t.sync()
        out, state = out.cpu().numpy(), state.cpu().numpy()
        seen = _replay(t, d_frames, table, starts, out, state, 1, 6, None, 0.5)
        assert 1 in seen and len(seen) > 1, seen
        for s in range(1, nf):                                    # assigned targets keep their distance
            p, st = out[0, :, s].astype(np.int64), state[0, :, s]
            for a in range(3):
                for b in range(a + 1, 3):
                    assert st[a] < 1 or st[b] < 1 or ((p[a] - p[b]) ** 2).sum() >= 25 * 25, (s, p, st)
    finally:
        t.close()


# ---- one target, far-apart targets ----
@pytest.mark.parametrize("first", [0, 1])
def test_one_target_per_group_is_the_indexed_chain(bt, stack, first):
    _, d_frames = stack
    table = np.array([[41 * c + f for f in range(10, 30)] for c in range(3)], np.int32)
    table[2, 15:] = -1
    starts = np.stack([_targets(c, 10, 1, c) for c in range(3)])          # [3, 1, 2]: a disc's centre each
    want = bt.detect_chains_indexed(d_frames, table, _cuda(starts[:, 0]), first=first)
    out, state = bt.detect_chains_exclusive(d_frames, table, _cuda(starts), first=first)
    bt.sync()
    assert np.array_equal(out.cpu().numpy()[:, 0], want.cpu().numpy())
    st = state.cpu().numpy()[:, 0]
    expect = np.ones_like(st)
    expect[:, 0] = 0 if first else 1
    expect[2, 15:] = 0
    assert np.array_equal(st, expect)


def test_far_apart_targets_walk_their_independent_chains(bt, stack):
    """Frames 0 ... 12 of "passing": the discs are 54 or more columns apart, no window sees the other one."""
    _, d_frames = stack
    table = np.arange(41, 54, dtype=np.int32)
    starts = np.array(es.scene("passing").truth[0], np.int32)
    want = bt.detect_chains_indexed(d_frames, np.tile(table, (2, 1)), _cuda(starts))
    out, state = bt.detect_chains_exclusive(d_frames, table[None], _cuda(starts[None]))
    bt.sync()
    assert np.array_equal(out.cpu().numpy()[0], want.cpu().numpy()) and (state.cpu().numpy() == 1).all()
    assert np.abs(out.cpu().numpy()[0, :, -1] - np.array(es.scene("passing").truth[12])).max() <= 1


# ---- the two scenes end to end ----
@pytest.mark.parametrize("name", list(es.SCENES))
def test_track_video_keeps_the_targets_apart(pt, name):
    sc = es.scene(name)
    d_frames = _cuda(sc.frames)
    args = dict(rate=24, start=0, stop=es.NF / 24, fps=24, target_width=es.TW, window_size=sc.ws[0],
                start_locations=[("ij", c) for c in sc.starts])
    ts, idx, state = pt.track_video(d_frames, exclusive=True, min_ratio=es.RATIO, min_distance=es.MIN_DISTANCE, **args)
    assert idx.shape == (2, es.NF, 2) and state.shape == (2, es.NF) and len(ts) == es.NF
    idx, state = idx.cpu().numpy(), state.cpu().numpy()
    track = [[tuple(int(v) for v in idx[t, k]) for t in range(2)] for k in range(es.NF)]
    states = [[int(state[t, k]) for t in range(2)] for k in range(1, es.NF)]
    assert (state[:, 0] == 0).all() and track[0] == sc.starts
    # both discs are tracked at the end: one target per disc, each within 1 px of its centre
    assert es.errors(track, sc.truth)[-1] <= 1, (name, track[-1])
    d2 = es.min_assigned_distance2(track, states)
    assert d2 is not None and d2 >= es.MIN_DISTANCE ** 2
    above = es.steps_above(track, sc.truth)
    print(name, "steps above 3 px:", above, "final:", track[-1], "states:", sorted({s for st in states for s in st}))
    assert above <= es.GPU_STEPS_ABOVE_3PX, (name, above)
    # the failing behaviour, pinned: independent chains end on one disc
    ts2, plain = pt.track_video(d_frames, **args)
    plain = plain.cpu().numpy()
    assert np.array_equal(ts, ts2) and tuple(plain[0, -1]) == tuple(plain[1, -1]), (name, plain[:, -1])
    assert min(np.abs(plain[0, -1] - np.array(c)).max() for c in sc.truth[-1]) <= 1
    assert es.steps_above([[tuple(plain[t, k]) for t in range(2)] for k in range(es.NF)], sc.truth) >= 20
    # subpixel and the overlay work on the positions as before
    seen = []
    res = pt.track_video(d_frames, exclusive=True, subpixel=True, diagnostic=lambda k0, ov: seen.append((k0, int(ov.shape[0]))), **args)
    assert len(res) == 4 and np.array_equal(res[1].cpu().numpy(), idx) and np.array_equal(res[3].cpu().numpy(), state)
    assert res[2].shape == (2, es.NF, 2) and sum(n for _, n in seen) == es.NF - 1


# ---- errors, repeat calls ----
def test_bad_arguments_launch_nothing(pt, bt, stack):
    import torch
    from pawsometracker_jl_amd import _lib
    _, d_frames = stack
    L = pt.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    G, T, k, ns = 2, 3, 4, 5
    table = np.array([[0, 1, 2, 3, 4], [41, 42, 43, -1, -1]], np.int32)
    starts = _cuda(np.stack([_targets(c, 0, T, c) for c in range(G)]))
    out = torch.zeros((G, T, ns, 2), dtype=torch.int32, device="cuda")
    state = torch.zeros((G, T, ns), dtype=torch.int32, device="cuda")
    ok = dict(t=bt._h, f=P(d_frames), fs=d_frames.stride(0), rs=d_frames.stride(1), nf=d_frames.shape[0], tab=table, ns=ns, G=G, T=T,
              first=0, k=k, md=0, rho=0.5, st=P(starts), o=P(out), s=P(state))

    def walk(**kw):
        a = dict(ok, **kw)
        tab = None if a["tab"] is None else C.c_void_p(np.ascontiguousarray(a["tab"], np.int32).ctypes.data)
        return L.pdog_detect_chains_exclusive(a["t"], a["f"], a["fs"], a["rs"], a["nf"], tab, a["ns"], a["G"], a["T"], a["first"],
                                              a["k"], a["md"], a["rho"], a["st"], a["o"], a["s"])

    bt.sync()
    before = (bt.exclusive_counts(), bt.peaks_counts())
    bad_entry, gap = table.copy(), table.copy()
    bad_entry[0, 2] = d_frames.shape[0]
    gap[1, 4] = 44                                               # a non-negative entry behind a negative one
    for kw in (dict(t=None), dict(f=None), dict(tab=None), dict(st=None), dict(o=None), dict(s=None), dict(T=0), dict(T=33), dict(k=33),
               dict(rho=-0.1), dict(rho=1.5), dict(rho=float("nan")), dict(G=0), dict(ns=0), dict(nf=0), dict(first=2),
               dict(rs=es.W - 1), dict(rs=_lib.PDOG_MAX_ROW_STRIDE + 1), dict(fs=-1), dict(tab=bad_entry), dict(tab=gap)):
        assert walk(**kw) == _lib.PDOG_E_ARG, kw
        assert L.pdog_last_error() != b""
    prev, ij = torch.zeros((G, T, 2), dtype=torch.int32, device="cuda"), torch.zeros((G, T, k, 2), dtype=torch.int32, device="cuda")
    peak, count = torch.ones((G, T, k), device="cuda"), torch.ones((G, T), dtype=torch.int32, device="cuda")
    o2, s2 = torch.zeros((G, T, 2), dtype=torch.int32, device="cuda"), torch.zeros((G, T), dtype=torch.int32, device="cuda")
    aok = [bt._h, G, T, k, 0, 0.5, P(prev), P(ij), P(peak), P(count), P(o2), P(s2)]
    for pos, v in ((0, None), (1, 0), (2, 0), (2, 33), (3, 0), (3, 33), (5, -0.5), (5, 2.0), (5, float("nan")), (6, None), (7, None),
                   (8, None), (9, None), (10, None), (11, None)):
        a = list(aok)
        a[pos] = v
        assert L.pdog_assign_exclusive(*a) == _lib.PDOG_E_ARG, (pos, v)
    bt.sync()                                                    # clean: nothing was launched
    assert (bt.exclusive_counts(), bt.peaks_counts()) == before
    assert int(out.abs().sum()) == 0 and int(state.abs().sum()) == 0 and int(s2.abs().sum()) == 0
    # the Python layer judges its arguments before any address reaches the library
    for exc, call in ((ValueError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, k=33)),
                      (TypeError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, k=2.0)),
                      (ValueError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, min_ratio=1.5)),
                      (TypeError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, min_ratio="1")),
                      (ValueError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, min_distance=0)),
                      (ValueError, lambda: bt.detect_chains_exclusive(d_frames, table, starts, first=2)),
                      (ValueError, lambda: bt.detect_chains_exclusive(d_frames, table[:1], starts)),
                      (TypeError, lambda: bt.detect_chains_exclusive(d_frames, table, starts.cpu())),
                      (TypeError, lambda: bt.detect_chains_exclusive(d_frames, table, starts[:, 0])),
                      (TypeError, lambda: bt.detect_chains_exclusive(d_frames.cpu(), table, starts)),
                      (TypeError, lambda: bt.assign_exclusive(prev, ij, peak.double(), count)),
                      (ValueError, lambda: bt.assign_exclusive(prev, ij, peak[:, :, :2].contiguous(), count)),
                      (ValueError, lambda: bt.assign_exclusive(prev, ij, peak, count, min_ratio=-1)),
                      (TypeError, lambda: bt.assign_exclusive(prev.cpu(), ij, peak, count)),
                      (TypeError, lambda: bt.assign_exclusive(prev[0], ij, peak, count))):
        with pytest.raises(exc):
            call()
    bt.sync()
    assert (bt.exclusive_counts(), bt.peaks_counts()) == before
    assert walk() == _lib.PDOG_OK                                # and the tracker works afterwards
    bt.sync()
    assert bt.exclusive_counts()[0] == before[0][0] + 5 and int(state[0].abs().sum()) > 0 and int(state[1, :, 3:].abs().sum()) == 0


def test_a_repeated_call_allocates_nothing(bt, stack):
    import torch
    _, d_frames = stack
    table = np.array([[41 * c + f for f in range(15, 25)] for c in range(3)], np.int32)
    starts = _cuda(np.stack([_targets(c, 15, 8, c) for c in range(3)]))
    one = bt.detect_chains_exclusive(d_frames, table, starts, first=1)
    bt.sync()
    torch.cuda.synchronize()
    counts = bt.exclusive_counts()
    import pawsometracker_jl_amd as m
    L, P = m.lib(), lambda t: C.c_void_p(t.data_ptr())
    out, state = torch.zeros_like(one[0]), torch.zeros_like(one[1])
    free = torch.cuda.mem_get_info()[0]
    assert L.pdog_detect_chains_exclusive(bt._h, P(d_frames), d_frames.stride(0), d_frames.stride(1), d_frames.shape[0],
                                          C.c_void_p(table.ctypes.data), 10, 3, 8, 1, 0, 0, 0.5, P(starts), P(out), P(state)) == 0
    bt.sync()
    after = bt.exclusive_counts()
    assert after[1] == counts[1] and after[0] == counts[0] + 9          # no workspace grew; nine joint steps
    assert torch.cuda.mem_get_info()[0] == free                          # nor did anything else in the library allocate
    assert torch.equal(out, one[0]) and torch.equal(state, one[1])
