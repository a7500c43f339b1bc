"""The predicted chain on the GPU (include/pawsome_predict.h): pdog_detect_chains_predicted on every path it can take — the fused
kernel's compile-time and runtime-length instances, the persistent roll chain, the fallback to the stepped motion walk — with
the path confirmed by pdog_get_predict_counts.  Positions, states and the final mstate are compared exactly: with
detect_chains_motion at one target per group and k = 1, and with tests/predict_restatement.py over the oracle's Float64 maps.
The scenes are tests/motion_scenes.py's "fast" and "vanish" (17 frames of 100 x 140, 11 x 11 windows): their responses are a
disc's or exactly 0, far from min_response on either side; one test adds noise, so that assigned frames are near-ties and the
kernels file them behind exact mode's refinement.  The whole file fails on a library without the symbols."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusive_scenes as es  # noqa: E402
import motion_scenes as ms  # noqa: E402
import predict_restatement as prs  # noqa: E402

pytestmark = pytest.mark.gpu
HW = (ms.H, ms.W)
NF = ms.FAST_NF
POISON = -77
IMAX = 2**31 - 1

# what a path needs: target width (10: l = 29, a compile-time length of both kernel families; 8: l = 21, the fused kernel's
# runtime-length instance), window, a pinned variant (129: the roll instance of l = 29), and the counter that must move
PATHS = {
    "fused_compile_time": dict(tw=10, ws=11, counter=0),
    "fused_runtime_length": dict(tw=8, ws=11, counter=0),
    "persistent": dict(tw=10, ws=11, variant=129, counter=1),
    "fallback_single_step": dict(tw=10, ws=11, single=True, counter=2),
    "fallback_window": dict(tw=10, ws=101, counter=2),          # a tile the fused kernel's LDS does not hold
}


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    assert hasattr(m.lib(), "pdog_detect_chains_predicted")
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scene_frames(name, tw):
    """The scene's 17 frames with a disc of radius tw // 2 (tw = 10: the scene's own frames)."""
    frames = np.stack([es.draw(HW, [((50, 15 + ms.FAST_SPEED * f), 0)], radius=tw // 2) for f in range(NF)])
    if name == "vanish":
        frames[ms.VANISH_FROM:] = ms.BKGD
    if tw == ms.TW:
        assert np.array_equal(frames, ms.scene(name).frames)
    return frames


@pytest.fixture(scope="module")
def trackers(pt):
    made = {}

    def get(path):
        if path not in made:
            cfg = PATHS[path]
            bt = pt.BatchTracker(ms.H, ms.W, cfg["tw"], (cfg["ws"], cfg["ws"]), True, ms.BKGD)
            if "variant" in cfg:
                bt.set_variant(cfg["variant"])
            made[path] = bt
        return made[path]
    yield get
    for t in made.values():
        t.close()


@pytest.fixture(scope="module")
def reference(oracle):
    """The Float64 restatement's walks, computed once per (target width, window, frames — named by `tag` —, row, start, m, coast,
    first, mstate)."""
    cache = {}

    def walk(tw, ws, tag, frames, row, start, m, coast, first=0, mstate=None):
        key = (tw, ws, tag, frames.shape, tuple(int(v) for v in row), tuple(int(v) for v in start), m, coast, first,
               None if mstate is None else tuple(int(v) for v in mstate))
        if key not in cache:
            Kn = oracle.dog_kernel(oracle.sigma(tw), True)
            cache[key] = prs.walk(oracle, frames, ms.BKGD, Kn, (ws // 2, ws // 2), row, start, m, coast, first, mstate)
        return cache[key]
    return walk


def _raw(pt, bt, d_frames, table, d_starts, m, coast, first, d_out, d_state, d_mstate):
    """The entry point itself, on the caller's (poisoned) outputs."""
    table = np.ascontiguousarray(table, np.int32)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = pt.lib().pdog_detect_chains_predicted(bt._h, P(d_frames), d_frames.stride(0), d_frames.stride(1), d_frames.shape[0], C.c_void_p(table.ctypes.data),
                                               table.shape[1], table.shape[0], first, m, coast, P(d_starts), P(d_out), P(d_state), P(d_mstate))
    assert rc == 0, pt.lib().pdog_last_error()


def _motion(bt, d_frames, table, d_starts, m, coast, first, mstate=None):
    """detect_chains_motion with every clip a group of one target and k = 1: (out [n, ns, 2], state [n, ns], mstate [n, 4])."""
    ms0 = None if mstate is None else mstate.clone().unsqueeze(1).contiguous()
    out, state, mst = bt.detect_chains_motion(d_frames, table, d_starts.unsqueeze(1).contiguous(), 1, None, 0.5, m, coast, first=first, mstate=ms0)
    return out[:, 0], state[:, 0], mst[:, 0]


# ---- every path, both scenes, exact mode on and off ----
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fp32"])
@pytest.mark.parametrize("name", ["fast", "vanish"])
@pytest.mark.parametrize("path", list(PATHS))
def test_paths_and_modes(pt, trackers, reference, path, name, exact):
    import torch
    cfg, sc = PATHS[path], ms.scene(name)
    bt = trackers(path)
    bt.set_exact(1 if exact else 0)
    try:
        frames = _scene_frames(name, cfg["tw"])
        d_frames = _cuda(frames)
        table = np.arange(NF, dtype=np.int32)[None]
        starts = _cuda(np.array(sc.starts, np.int32))
        m, coast = sc.min_response, sc.coast
        before, refined0 = bt.predict_counts(), bt.exact_stats()[2]
        if cfg.get("single"):         # a table of one step per call, continued through mstate: 16 walks the stepped path takes
            outs, states, mstate, cur = [starts.clone()[:, None]], [torch.zeros((1, 1), dtype=torch.int32, device="cuda")], None, starts
            for f in range(1, NF):
                o, s, mstate = bt.detect_chains_predicted(d_frames, table[:, f:f + 1], cur, m, coast, mstate)
                cur = o[:, 0].contiguous()
                outs.append(o)
                states.append(s)
            out, state, calls = torch.cat(outs, 1), torch.cat(states, 1), NF - 1
        else:
            out, state, mstate = bt.detect_chains_predicted(d_frames, table, starts, m, coast, first=1)
            calls = 1
        bt.sync()
        after, refined1 = bt.predict_counts(), bt.exact_stats()[2]
        moved = [a - b for a, b in zip(after, before)]
        assert moved[:3] == [calls if c == cfg["counter"] else 0 for c in range(3)], (path, moved)
        want = _motion(bt, d_frames, table, starts, m, coast, 1)
        bt.sync()
        refined2 = bt.exact_stats()[2]
        out, state, mstate = out.cpu().numpy(), state.cpu().numpy(), mstate.cpu().numpy()
        print(path, name, "exact" if exact else "fp32", "final", out[0, -1], "states", state[0].tolist(), "mstate", mstate[0].tolist(), "refined", refined1 - refined0)
        for got, w, what in zip((out, state, mstate), want, ("positions", "states", "mstate")):
            assert np.array_equal(got, w.cpu().numpy()), (path, name, what, got, w)
        ref = reference(cfg["tw"], cfg["ws"], name, frames, table[0], sc.starts[0], m, coast, 1)
        for got, w, what in zip((out[0], state[0], mstate[0]), ref, ("positions", "states", "mstate")):
            assert np.array_equal(got, w), (path, name, what, got, w)
        track = [[tuple(int(v) for v in p)] for p in out[0]]
        scene_as_it_is = cfg["tw"] == ms.TW and cfg["ws"] == ms.FAST_WS
        if name == "vanish":
            assert track[ms.VANISH_FROM:] == [[p] for p in ms.VANISH_TAIL] or not scene_as_it_is
            assert state[0].tolist() == [0] + [1] * (ms.VANISH_FROM - 1) + [-1] * (NF - ms.VANISH_FROM)
            if exact and cfg["counter"] < 2:
                # a held frame is not refined: the eight flat frames (every response ties at 0) add nothing to the walk's first nine
                bt.detect_chains_predicted(d_frames, table[:, :ms.VANISH_FROM], starts, m, coast, first=1)
                bt.sync()
                assert bt.exact_stats()[2] - refined2 == refined1 - refined0
        else:
            assert (max(ms.errors_true(track, sc.truth)) <= 3 or not scene_as_it_is) and (state[0, 1:] == 1).all()
    finally:
        bt.set_exact(1)


# ---- near-ties: an assigned frame is filed after exact mode's refinement, or after the flag was withdrawn ----
@pytest.mark.parametrize("mode", [1, 2], ids=["exact", "refine_everything"])
@pytest.mark.parametrize("path", ["fused_compile_time", "fused_runtime_length", "persistent"])
def test_noisy_frames_are_refined_like_the_motion_walk(pt, trackers, path, mode):
    """"fast" under +-2 levels of seeded noise, one clip on the disc and two on noise alone (min_response 0: noise is assigned).
    With set_exact(2) every assigned window is refined — the kernel files it behind the refinement —; with exact mode on, flagged
    windows are refined or, where their own |pixel - dc| bound says so, withdrawn.  The stepped motion walk refines the same
    windows by the same arithmetic: positions, states and mstate are equal."""
    cfg = PATHS[path]
    bt = trackers(path)
    rng = np.random.default_rng(7)
    clean = _scene_frames("fast", cfg["tw"]).astype(np.int16)
    frames = np.where(clean == 0, 0, clean + rng.integers(-2, 3, clean.shape)).astype(np.uint8)
    d_frames = _cuda(frames)
    table = np.tile(np.arange(NF, dtype=np.int32), (3, 1))
    starts = _cuda(np.array([(50, 15), (20, 70), (85, 30)], np.int32))
    bt.set_exact(mode)
    try:
        refined0 = bt.exact_stats()[2]
        out, state, mstate = bt.detect_chains_predicted(d_frames, table, starts, 0.0, 3, first=1)
        bt.sync()
        refined = bt.exact_stats()[2] - refined0
        want = _motion(bt, d_frames, table, starts, 0.0, 3, 1)
        bt.sync()
        print(path, "mode", mode, "refined", refined, "states", sorted(set(state.cpu().numpy().ravel().tolist())), "final", out[:, -1].cpu().numpy().tolist())
        assigned = int((state == 1).sum())
        assert assigned >= 16 and (refined == assigned if mode == 2 else refined <= assigned)
        for got, w, what in zip((out, state, mstate), want, ("positions", "states", "mstate")):
            assert np.array_equal(got.cpu().numpy(), w.cpu().numpy()), (path, mode, what, got, w)
        track = [[tuple(int(v) for v in p)] for p in out[0].cpu().numpy()]
        assert max(ms.errors_true(track, ms.scene("fast").truth)) <= 3 or cfg["tw"] != ms.TW
    finally:
        bt.set_exact(1)


# ---- many clips: more than stay resident, so a workgroup of the fused kernel walks several ----
ROWS = [list(range(NF)), [-1] * NF, [3] + [-1] * (NF - 1), [0, 1, 2, 2, 2, 3, 4, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13], list(range(0, NF, 2)) + [-1] * 8,
        list(range(9)) + [-1] * 8, list(range(NF - 1, -1, -1)), [5, 6, 7, 8, 9, 10, 11] + [-1] * 10, [0, 1] + [-1] * 15, [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 16]]


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("path", ["fused_compile_time", "persistent"])
def test_many_clips_share_the_frames(pt, trackers, reference, path, first):
    """1024 clips over ONE stack of 34 frames ("fast", then "vanish"): even clips walk "fast", odd clips "vanish", each on one of ten
    rows drawn by a seeded generator — lengths 0, 1, 2, 7, 9 and 17, repeated frames, every second frame, the frames backwards.
    A clip that inherited the carry of the clip its workgroup walked before it (a velocity of 7, a hold count) starts its first
    window somewhere else and files other positions.  Outputs past a row's end keep their poison, and a clip without a step
    keeps its mstate."""
    import torch
    bt = trackers(path)
    n = 1024
    rng = np.random.default_rng(20261020 + first)
    pick = rng.integers(0, len(ROWS), n)
    pick[:2 * len(ROWS)] = np.repeat(np.arange(len(ROWS)), 2)             # every (scene, row) occurs
    stack = np.concatenate([_scene_frames("fast", 10), _scene_frames("vanish", 10)])
    table = np.array([[f + NF * (c & 1) if f >= 0 else -1 for f in ROWS[pick[c]]] for c in range(n)], np.int32)
    lens = (table >= 0).sum(1)
    starts = np.array([(50, 15 + ms.FAST_SPEED * max(ROWS[pick[c]][0], 0)) for c in range(n)], np.int32)
    steps = lens > first
    mstate0 = np.where(steps[:, None], 0, 5).astype(np.int32) * np.ones((1, 4), np.int32)
    d_stack, d_starts = _cuda(stack), _cuda(starts)
    out = torch.full((n, NF, 2), POISON, dtype=torch.int32, device="cuda")
    state = torch.full((n, NF), POISON, dtype=torch.int32, device="cuda")
    mstate = _cuda(mstate0)
    m, coast = ms.VANISH_MIN_RESPONSE, ms.VANISH_COAST
    before = bt.predict_counts()
    _raw(pt, bt, d_stack, table, d_starts, m, coast, first, out, state, mstate)
    bt.sync()
    moved = [a - b for a, b in zip(bt.predict_counts(), before)]
    assert moved[:3] == [1 if c == PATHS[path]["counter"] else 0 for c in range(3)], moved
    out, state, mstate = out.cpu().numpy(), state.cpu().numpy(), mstate.cpu().numpy()
    for c in range(n):                                                           # rows past len are untouched
        assert (out[c, lens[c]:] == POISON).all() and (state[c, lens[c]:] == POISON).all(), c
    assert np.array_equal(mstate[~steps], mstate0[~steps]) and (mstate[steps][:, 3] == 0).all()
    # the Float64 restatement, once per (scene, row)
    seen = set()
    for c in range(n):
        ref = reference(10, 11, "fast+vanish", stack, table[c], starts[c], m, coast, first, mstate0[c])
        L = lens[c]
        assert np.array_equal(out[c, :L], ref[0][:L]) and np.array_equal(state[c, :L], ref[1][:L]) and np.array_equal(mstate[c], ref[2]), (c, pick[c], out[c], ref)
        seen |= set(state[c, :L].tolist())
    assert seen == ({-1, 0, 1} if first else {-1, 1})
    # and the stepped motion walk, bit for bit (its own outputs are zeroed past a row's end)
    want = _motion(bt, d_stack, table, d_starts, m, coast, first, _cuda(mstate0))
    bt.sync()
    valid = np.arange(NF)[None] < lens[:, None]
    assert np.array_equal(np.where(valid[..., None], out, 0), want[0].cpu().numpy()) and np.array_equal(np.where(valid, state, 0), want[1].cpu().numpy())
    assert np.array_equal(mstate, want[2].cpu().numpy())
    # a second call of the same sizes stages nothing new
    grown = bt.predict_counts()[3]
    free = torch.cuda.mem_get_info()[0]
    _raw(pt, bt, d_stack, table, d_starts, m, coast, first, torch.empty_like(want[0]), torch.empty_like(want[1]), None)
    bt.sync()
    assert bt.predict_counts()[3] == grown and torch.cuda.mem_get_info()[0] == free


# ---- a walk split inside the coast equals the one-call walk ----
@pytest.mark.parametrize("path", ["fused_compile_time", "fused_runtime_length", "persistent", "fallback_window"])
def test_continuation(pt, trackers, path):
    import torch
    cfg, sc = PATHS[path], ms.scene("vanish")
    bt = trackers(path)
    d_frames = _cuda(_scene_frames("vanish", cfg["tw"]))
    table = np.arange(NF, dtype=np.int32)[None]
    starts = _cuda(np.array(sc.starts, np.int32))
    m, coast = sc.min_response, sc.coast
    one = bt.detect_chains_predicted(d_frames, table, starts, m, coast, first=1)
    a = bt.detect_chains_predicted(d_frames, table[:, :6], starts, m, coast, first=1)                                # steps 0 ... 5
    b = bt.detect_chains_predicted(d_frames, table[:, 6:11], a[0][:, -1].contiguous(), m, coast, a[2])                # 6 ... 10: held from 9 on
    assert b[2] is a[2]                                                                                               # updated in place
    mid = b[2].clone()
    c = bt.detect_chains_predicted(d_frames, table[:, 11:], b[0][:, -1].contiguous(), m, coast, b[2])                 # 11 is the coast's last step
    bt.sync()
    assert mid.cpu().numpy().tolist() == [[0, ms.FAST_SPEED, 2, 0]]                                                  # split INSIDE the coast
    assert torch.equal(torch.cat([a[0], b[0], c[0]], 1), one[0]) and torch.equal(torch.cat([a[1], b[1], c[1]], 1), one[1]) and torch.equal(c[2], one[2])


# ---- the frame's border, the corners, a state at the ends of int32 ----
@pytest.mark.parametrize("path", ["fused_compile_time", "fused_runtime_length", "persistent"])
def test_edges(pt, trackers, reference, path):
    """Nine frames whose disc runs out of the frame along row 3 — (3, 104 + 7 f), gone after frame 6 —, walked by five clips: one
    on the disc, one from (1, 1), one from (h, w), and two whose mstate holds v = +-(2^31 - 1) with n_held = INT32_MAX and 0: their
    first windows lie in opposite corners, wherever p + v would have overflowed to."""
    cfg = PATHS[path]
    bt = trackers(path)
    frames = np.stack([es.draw(HW, [((3, 104 + 7 * f), 0)], radius=cfg["tw"] // 2) for f in range(9)])
    assert (frames[7] == ms.BKGD).all() and (frames[5] != ms.BKGD).any()
    table = np.tile(np.arange(9, dtype=np.int32), (5, 1))
    starts = np.array([(3, 104), (1, 1), (ms.H, ms.W), (50, 70), (3, 104)], np.int32)
    mstate0 = np.array([[0, 7, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [IMAX, -IMAX, IMAX, 9], [-IMAX, IMAX, 0, 9]], np.int32)
    d_frames, d_starts = _cuda(frames), _cuda(starts)
    m, coast = 1e-3, 2
    out, state, mstate = bt.detect_chains_predicted(d_frames, table, d_starts, m, coast, _cuda(mstate0))
    want = _motion(bt, d_frames, table, d_starts, m, coast, 0, _cuda(mstate0))
    bt.sync()
    out, state, mstate = out.cpu().numpy(), state.cpu().numpy(), mstate.cpu().numpy()
    print(path, "on the disc:", out[0].tolist(), state[0].tolist(), "corners:", out[1, -1], out[2, -1], out[3, 0], out[4, 0])
    for got, w, what in zip((out, state, mstate), want, ("positions", "states", "mstate")):
        assert np.array_equal(got, w.cpu().numpy()), (path, what, got, w)
    for c in range(5):
        ref = reference(cfg["tw"], cfg["ws"], "edge", frames, table[c], starts[c], m, coast, 0, mstate0[c])
        assert np.array_equal(out[c], ref[0]) and np.array_equal(state[c], ref[1]) and np.array_equal(mstate[c], ref[2]), (path, c, out[c], ref)
    assert state[0, 0] == 1 and state[0, -1] == -1 and (out >= 1).all() and (out[..., 0] <= ms.H).all() and (out[..., 1] <= ms.W).all()
    assert tuple(out[3, 0]) == (ms.H, 1) and tuple(out[4, 0]) == (1, ms.W) and (state[1:4] == -1).all()


# ---- errors: PDOG_E_ARG with nothing launched ----
def test_bad_arguments_launch_nothing(pt, trackers):
    import torch
    from pawsometracker_jl_amd import _lib
    bt = trackers("fused_compile_time")
    L, P = pt.lib(), lambda t: C.c_void_p(t.data_ptr())
    d_frames = _cuda(_scene_frames("fast", 10))
    table = np.array([[0, 1, 2, 3, 4], [5, 6, 7, -1, -1]], np.int32)
    starts = _cuda(np.full((2, 2), 50, np.int32))
    out = torch.full((2, 5, 2), POISON, dtype=torch.int32, device="cuda")
    state = torch.full((2, 5), POISON, dtype=torch.int32, device="cuda")
    mstate = torch.full((2, 4), 3, dtype=torch.int32, device="cuda")
    ok = dict(t=bt._h, f=P(d_frames), fs=d_frames.stride(0), rs=d_frames.stride(1), nf=NF, tab=table, ns=5, nc=2, first=0, m=0.0, coast=2,
              st=P(starts), o=P(out), s=P(state), ms=P(mstate))

    def walk(**kw):
        a = dict(ok, **kw)
        tab = None if a["tab"] is None else C.c_void_p(np.ascontiguousarray(a["tab"], np.int32).ctypes.data)
        return L.pdog_detect_chains_predicted(a["t"], a["f"], a["fs"], a["rs"], a["nf"], tab, a["ns"], a["nc"], a["first"], a["m"], a["coast"],
                                              a["st"], a["o"], a["s"], a["ms"])

    bt.sync()
    before = (bt.predict_counts(), bt.motion_counts(), bt.peaks_counts())
    bad_entry, bad_tail = table.copy(), table.copy()
    bad_entry[0, 2] = NF
    bad_tail[1, 4] = 0                                                 # a frame behind a negative entry
    for kw in (dict(t=None), dict(f=None), dict(tab=None), dict(st=None), dict(o=None), dict(s=None), dict(m=-0.5), dict(m=float("nan")),
               dict(m=float("inf")), dict(m=-float("inf")), dict(coast=-1), dict(nc=0), dict(nc=-1), dict(ns=0), dict(nf=0), dict(first=2), dict(first=-1),
               dict(rs=ms.W - 1), dict(fs=-1), dict(tab=bad_entry), dict(tab=bad_tail), dict(nc=2**16, ns=2**15)):
        assert walk(**kw) == _lib.PDOG_E_ARG, kw
        assert L.pdog_last_error() != b""
    assert L.pdog_get_predict_counts(bt._h, None) == _lib.PDOG_E_ARG
    bt.sync()                                                    # clean: nothing was launched
    assert (bt.predict_counts(), bt.motion_counts(), bt.peaks_counts()) == before
    assert bool((out == POISON).all()) and bool((state == POISON).all()) and bool((mstate == 3).all())
    for exc, call in ((ValueError, lambda: bt.detect_chains_predicted(d_frames, table, starts, coast=-1)),
                      (TypeError, lambda: bt.detect_chains_predicted(d_frames, table, starts, coast=1.0)),
                      (ValueError, lambda: bt.detect_chains_predicted(d_frames, table, starts, min_response=-1)),
                      (ValueError, lambda: bt.detect_chains_predicted(d_frames, table, starts, first=2)),
                      (ValueError, lambda: bt.detect_chains_predicted(d_frames, table, starts[:1])),
                      (ValueError, lambda: bt.detect_chains_predicted(d_frames, table, starts, mstate=mstate[:1])),
                      (TypeError, lambda: bt.detect_chains_predicted(d_frames, table, starts, mstate=mstate.cpu())),
                      (TypeError, lambda: bt.detect_chains_predicted(d_frames, table, starts.cpu()))):
        with pytest.raises(exc):
            call()
    bt.sync()
    assert (bt.predict_counts(), bt.motion_counts(), bt.peaks_counts()) == before
    mstate.zero_()
    assert walk() == _lib.PDOG_OK                                # and the tracker works afterwards
    bt.sync()
    assert bt.predict_counts()[0] == before[0][0] + 1 and bool((state[0] != POISON).all()) and bool((state[1, 3:] == POISON).all())
    assert bool((out[1, 3:] == POISON).all()) and bool((mstate[:, 3] == 0).all())


# ---- end to end ----
def test_track_video_with_predicted_chains(pt, trackers):
    import torch
    sc = ms.scene("vanish")
    d_frames = _cuda(sc.frames)
    locs = [("ij", sc.starts[0]), ("ij", (20, 70))]             # the second target sits where nothing ever comes
    args = dict(rate=24, start=0, stop=NF / 24, fps=24, target_width=ms.TW, window_size=ms.FAST_WS, start_locations=locs)
    ts, idx, state = pt.track_video(d_frames, predict=True, coast=sc.coast, min_response=sc.min_response, **args)
    assert idx.shape == (2, NF, 2) and state.shape == (2, NF) and len(ts) == NF
    bt = trackers("fused_compile_time")
    out, st, _ = bt.detect_chains_predicted(d_frames, np.tile(np.arange(NF, dtype=np.int32), (2, 1)), idx[:, 0].contiguous(), sc.min_response, sc.coast, first=1)
    bt.sync()
    assert torch.equal(idx, out) and torch.equal(state, st) and bool((state[:, 0] == 0).all())
    assert [tuple(int(v) for v in p) for p in idx[0, ms.VANISH_FROM:].cpu().numpy()] == ms.VANISH_TAIL
    assert bool((state[1, 1:] == -1).all()) and bool((idx[1] == idx[1, :1]).all())          # lost from the start: it waits where it is
    ts2, plain = pt.track_video(d_frames, **args)                                             # without the keyword: as before
    assert np.array_equal(ts, ts2) and plain.shape == idx.shape
    seen = []
    res = pt.track_video(d_frames, predict=True, subpixel=True, diagnostic=lambda k0, ov: seen.append((k0, int(ov.shape[0]))), **args)
    assert len(res) == 4 and res[2].shape == (2, NF, 2) and res[3].shape == (2, NF) and sum(k for _, k in seen) == NF - 1
