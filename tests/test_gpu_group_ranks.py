"""pdog_group_detect_batch with MORE THAN ONE RANK on one device.  GroupTracker.local (pdog_group_test_create_local) puts N
trackers on one GPU, each with its own stream, behind the same table of collective calls librccl fills for pdog_group_create;
the table's stand-in gather is stream-ordered (events, device-to-device copies on the root's stream) and checks the caller's
protocol (one Gather per rank between GroupStart and GroupEnd, same count, root 0, int32).  So these lines of
pdog_group_detect_batch run here with ndev > 1 for the first time: the pointer checks per shard, the grow path that drains every
rank, the per-rank launch loop with r > 0 and max_n != the shard's size, empty shards, per-rank n_frames / frame_index / frames,
the early return when a rank's pdog_detect_batch refuses, the grouped gather into d_gathered, group_compact_kernel on the root's
stream behind it, and pdog_group_sync with a flag raised on one rank only.  What still has NOT run: ncclCommInitAll over
distinct devices, RCCL's own gather between two GPUs (no byte has crossed xGMI), and bench.py --group with N > 1.

Every rank has a frame stack of its own (the scene's frames in another order, shifted, another number of them), guesses of its
own and a frame index of its own, and the oracle shows BEFORE anything runs that a shard run against another rank's frames,
guesses or index gives other positions.  Every comparison is exact: with the oracle (tests/layout_frames.py's scene
"l29 21x21": windows over every border) and, bit for bit, with BatchTracker.detect rank by rank.  Every `out` is preset to -1
and followed by 8 guard rows of -7.

Measured on an MI355X: the file's 15 tests take 4 s run alone, 2.5 s of them the first test's setup (torch and the library
start the device); the slowest test body, 4 x 4098 with the oracle on every window, 0.22 s, the others 0.01 … 0.11 s."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_frames as lf  # noqa: E402

pytestmark = pytest.mark.gpu

SCENE = "l29 21x21"
GUARD = 8
MAX_RANKS = 8
SHAPES = ((2, 8), (3, 10), (3, 11), (8, 8), (8, 5), (5, 3), (3, 1), (4, 4098))    # (ranks, n_total)


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- a frame stack, guesses and a frame index per rank ----
def n_frames_of(r):
    return 4 + r % 3


_FRAMES = {}


def rank_frames(sc, r):
    """Rank r's own stack: n_frames_of(r) frames, the scene's in an order rolled by r, each shifted (with wrap-around) by an
    amount of the rank's own — 6 rows or 7 columns apart from rank to rank, more than the scene's targets differ among
    themselves — and by one more pixel each time the scene's frames have been gone through: the targets move."""
    if (sc, r) not in _FRAMES:
        out = []
        for k in range(n_frames_of(r)):
            turn = k // sc.nf
            out.append(np.roll(sc.frames[(k + r) % sc.nf], (6 * (r % 3 - 1) + turn, 7 * (r // 3 % 3 - 1) - turn), axis=(0, 1)))
        _FRAMES[(sc, r)] = np.ascontiguousarray(np.stack(out))
    return _FRAMES[(sc, r)]


def _pos(sc, oracle, q, k, g):
    """The oracle's position for guess g on frame k of rank q's stack (memoised in the scene)."""
    return sc.position(oracle, int(k), (int(g[0]), int(g[1])), frames=rank_frames(sc, q), tag=("rank", q))


def plan(pt, sc, oracle, ranks, n_total, indexed, salt=0):
    """Per rank: the guesses of its shard, its frame index (indexed: a non-identity one, with repeats once the shard exceeds the
    stack; else None, window b on frame b) and the oracle's positions on ITS frames."""
    W = sc.windows
    P = SimpleNamespace(ranks=ranks, n_total=n_total, indexed=indexed, n=[], fi=[], g=[], frame_of=[], want=[])
    for r in range(ranks):
        lo, hi = pt.shard_range(n_total, r, ranks)
        n, nf, b = hi - lo, n_frames_of(r), np.arange(hi - lo)
        if indexed:
            e = (5 * r + salt + b) % len(W)
            fi = np.array([(W[i][0] + j // len(W) + r) % nf for j, i in enumerate(e)], np.int32)
            if n and np.array_equal(fi, b):
                fi[0] = (fi[0] + 1) % nf
            assert n == 0 or not np.array_equal(fi, b)
            assert n <= nf or len(set(fi.tolist())) < n
            frame_of = fi
        else:
            assert n <= nf, "frame_index None: the shard must fit the rank's frames"
            e = (5 * r + salt + 3 * b) % len(W)
            fi, frame_of = None, b
        g = np.array([W[i][1] for i in e], np.int32).reshape(n, 2)
        if n:       # the shard's first window is centred where the target lay before the rank's shift: where it lies now decides the answer
            g[0] = sc.centres[(int(frame_of[0]) + r) % sc.nf]
        P.n.append(n)
        P.fi.append(fi)
        P.g.append(g)
        P.frame_of.append(np.asarray(frame_of, np.int64))
        P.want.append(np.array([_pos(sc, oracle, r, k, q) for k, q in zip(frame_of, g)], np.int32).reshape(n, 2))
    assert sum(P.n) == n_total and max(P.n) - min(P.n) <= 1
    P.expect = np.concatenate(P.want)
    return P


def premise(sc, oracle, P):
    """From the oracle alone: rank r's windows on rank q's frames, with rank q's guesses, or through rank q's frame index give
    other positions than rank r's own.  Returns how many mix-ups were told apart."""
    told = 0
    for r in range(P.ranks):
        for q in range(P.ranks):
            m = min(P.n[r], P.n[q])
            if q == r or m == 0:
                continue
            own = P.want[r][:m].tolist()
            on_q_frames = [list(_pos(sc, oracle, q, k % n_frames_of(q), g)) for k, g in zip(P.frame_of[r][:m], P.g[r][:m])]
            assert on_q_frames != own, ("frames", r, q)
            assert not np.array_equal(P.g[q][:m], P.g[r][:m]) or m == 1, ("the guesses themselves", r, q)
            # (two windows that both hold the target give one answer: a shard of a single window need not tell the guesses apart)
            with_q_guesses = [list(_pos(sc, oracle, r, k, g)) for k, g in zip(P.frame_of[r][:m], P.g[q][:m])]
            assert with_q_guesses != own or m == 1, ("guesses", r, q)
            told += 1 + (with_q_guesses != own)
            if P.indexed and not np.array_equal(P.fi[q][:m] % n_frames_of(r), P.fi[r][:m]):
                through_q_index = [list(_pos(sc, oracle, r, k % n_frames_of(r), g)) for k, g in zip(P.fi[q][:m], P.g[r][:m])]
                assert through_q_index != own or m == 1, ("frame index", r, q)
                told += through_q_index != own
    return told


def upload(P):
    """The guesses and indices on the device and `out`: n_total rows of -1, then GUARD rows of -7."""
    import torch
    P.d_g = [_cuda(g) for g in P.g]
    P.d_fi = [_cuda(fi) for fi in P.fi] if P.indexed else None
    P.out_full = torch.full((P.n_total + GUARD, 2), -7, dtype=torch.int32, device="cuda:0")
    P.out_full[:P.n_total] = -1
    P.out = P.out_full[:P.n_total]
    return P


def verify(P, skip=()):
    got = P.out_full.cpu().numpy()
    assert (got[P.n_total:] == -7).all(), "the guard rows behind n_total were written"
    got = got[:P.n_total]
    assert not (got == -1).any(), ("rows that nothing wrote", np.nonzero((got == -1).any(axis=1))[0][:8])
    keep = np.ones(P.n_total, bool)
    keep[list(skip)] = False
    bad = np.nonzero((got != P.expect).any(axis=1) & keep)[0]
    assert bad.size == 0, (P.ranks, P.n_total, P.indexed, bad[:8], got[bad[:8]], P.expect[bad[:8]])
    return got


def untouched(P):
    got = P.out_full.cpu().numpy()
    return (got[:P.n_total] == -1).all() and (got[P.n_total:] == -7).all()


def twin(pt, sc, P, d_frames):
    """BatchTracker.detect rank by rank, on that rank's frames, guesses and index, concatenated in shard order."""
    import torch
    bt = pt.BatchTracker(sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)
    try:
        outs = [bt.detect(d_frames[r], P.d_g[r], frame_index=P.d_fi[r] if P.indexed else None) for r in range(P.ranks) if P.n[r]]
        bt.sync()
        return torch.cat(outs, 0).cpu().numpy()
    finally:
        bt.close()


def raw_detect(pt, gt, P, d_frames, out_ptr, null_frames=(), null_guesses=(), n_frames=None):
    """pdog_group_detect_batch through ctypes, with pointers and counts the Python layer would not let through."""
    PT = C.c_void_p * P.ranks
    fr = PT(*[None if r in null_frames else d_frames[r].data_ptr() for r in range(P.ranks)])
    gs = PT(*[None if r in null_guesses else (P.d_g[r].data_ptr() or None) for r in range(P.ranks)])
    fi = PT(*[(t.data_ptr() or None) for t in P.d_fi]) if P.indexed else None
    nf = (C.c_int * P.ranks)(*(n_frames or [d_frames[r].shape[0] for r in range(P.ranks)]))
    return pt.lib().pdog_group_detect_batch(gt._h, fr, d_frames[0].stride(0), d_frames[0].stride(1), nf, fi, gs, P.n_total, C.c_void_p(out_ptr))


@pytest.fixture(scope="module")
def sc():
    return lf.scene(SCENE)


@pytest.fixture(scope="module")
def d_frames(sc):
    """Every rank's stack on the device, contiguous, uploaded once."""
    import torch
    d = [_cuda(rank_frames(sc, r)) for r in range(MAX_RANKS)]
    assert len({f.shape[0] for f in d}) > 1                       # n_frames differs from rank to rank
    torch.cuda.synchronize()
    return d


def _group(pt, sc, ranks):
    return pt.GroupTracker.local(ranks, sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)


# ---- a. shard shapes ----
@pytest.mark.parametrize("ranks,n_total", SHAPES, ids=[f"{r}x{n}" for r, n in SHAPES])
def test_shard_shapes(pt, oracle, sc, d_frames, ranks, n_total):
    import torch
    modes = [True] + ([False] if -(-n_total // ranks) <= min(n_frames_of(r) for r in range(ranks)) else [])
    assert (len(modes) == 2) == (n_total < 4098)
    gt = _group(pt, sc, ranks)
    try:
        assert gt.size() == ranks and [gt.shard(n_total, r) for r in range(ranks)] == [pt.shard_range(n_total, r, ranks) for r in range(ranks)]
        for indexed in modes:
            P = upload(plan(pt, sc, oracle, ranks, n_total, indexed))
            told = premise(sc, oracle, P)
            assert told > 0 or sum(1 for n in P.n if n) < 2       # (3, 1): one shard, nothing to mix up
            for r in (0, ranks - 1):
                assert gt.kernel_for_batch(P.n[r], r) == 300
            torch.cuda.synchronize()
            gt.detect(d_frames[:ranks], P.d_g, n_total, P.out, frame_index=P.d_fi)
            gt.sync()
            got = verify(P)                                        # the oracle, on every window
            assert np.array_equal(got, twin(pt, sc, P, d_frames)), (ranks, n_total, indexed)
            for r in (0, ranks - 1):
                assert gt.kernel_for_batch(P.n[r], r) == 300
    finally:
        gt.close()


# ---- b. strided shards ----
def test_strided_shards(pt, oracle, sc, d_frames):
    """Every rank's frames behind the worst corner of the layout matrix (odd slack, odd base, odd gap; the same strides on every
    rank, as the entry point takes them) against the contiguous twin."""
    import torch
    ranks, n_total = 3, 11
    lays = [lf.make(rank_frames(sc, r), 19, 2 * sc.w + 5, 3 * sc.w + 7, sc.poison) for r in range(ranks)]
    d_str = [lf.to_device(lay) for lay in lays]
    assert len({(f.stride(0), f.stride(1)) for f in d_str}) == 1 and d_str[0].stride(1) == sc.w + 19
    gt = _group(pt, sc, ranks)
    try:
        outs = []
        for frames in (d_frames[:ranks], d_str):
            P = upload(plan(pt, sc, oracle, ranks, n_total, True))
            torch.cuda.synchronize()
            gt.detect(frames, P.d_g, n_total, P.out, frame_index=P.d_fi)
            gt.sync()
            outs.append(verify(P))
        assert np.array_equal(outs[0], outs[1])
        assert gt.kernel_for_batch(4, 0) == 300 and gt.kernel_for_batch(3, 2) == 300
    finally:
        gt.close()


# ---- c. one group, many calls, no sync in between ----
def test_back_to_back_calls_without_a_sync(pt, oracle, sc, d_frames):
    """10, 10 again with other guesses, 4 098 (the buffers grow: every rank is drained), 5 (unequal, behind d_gathered's stale
    contents), 9 (equal: gathered straight into out) on one 3-rank group; ONE sync at the end.  Then again with room reserved."""
    import torch
    ranks = 3
    calls = ((10, True, 0), (10, False, 7), (4098, True, 3), (5, True, 11), (9, True, 2))
    gt = _group(pt, sc, ranks)
    try:
        for reserved in (False, True):
            if reserved:
                gt.reserve(4098)
            plans = [upload(plan(pt, sc, oracle, ranks, n, indexed, salt)) for n, indexed, salt in calls]
            assert not np.array_equal(plans[0].expect, plans[1].expect)
            torch.cuda.synchronize()
            for P in plans:
                gt.detect(d_frames[:ranks], P.d_g, P.n_total, P.out, frame_index=P.d_fi)
            gt.sync()
            for P in plans:
                verify(P)
    finally:
        gt.close()


# ---- d. errors ----
def _spoil(sc, P, r, b):
    """Shard-local window b of rank r gets a guess one row beyond the padded frame; returns its window number."""
    P.g[r][b] = (sc.h + sc.l // 2 + 2, 10)
    return sum(P.n[:r]) + b


@pytest.mark.parametrize("bad_ranks", [(2,), (1, 2)], ids=["rank 2", "ranks 1 and 2"])
def test_a_guess_out_of_range_on_some_ranks(pt, oracle, sc, d_frames, bad_ranks):
    import torch
    ranks, n_total = 3, 10
    gt = _group(pt, sc, ranks)
    try:
        P = plan(pt, sc, oracle, ranks, n_total, True)
        skip = [_spoil(sc, P, r, 1) for r in bad_ranks]
        upload(P)
        torch.cuda.synchronize()
        gt.detect(d_frames[:ranks], P.d_g, n_total, P.out, frame_index=P.d_fi)
        with pytest.raises(pt.PdogError) as e:
            gt.sync()
        assert e.value.code == pt._lib.PDOG_E_RANGE and "BoundsError" in str(e.value)
        assert pt.lib().pdog_last_error().startswith(f"rank {bad_ranks[0]}:".encode()), pt.lib().pdog_last_error()
        gt.sync()                                                  # reported once, and every rank was cleared
        verify(P, skip=skip)                                       # the in-range windows of ALL ranks
        Q = upload(plan(pt, sc, oracle, ranks, n_total, True, salt=4))
        torch.cuda.synchronize()
        gt.detect(d_frames[:ranks], Q.d_g, n_total, Q.out, frame_index=Q.d_fi)
        gt.sync()
        verify(Q)
    finally:
        gt.close()


def test_null_pointers_per_rank(pt, oracle, sc, d_frames):
    import torch
    ranks = 3
    gt = _group(pt, sc, ranks)
    try:
        P = upload(plan(pt, sc, oracle, ranks, 10, True))
        torch.cuda.synchronize()
        for kw in (dict(null_frames=(1,)), dict(null_guesses=(1,))):
            assert raw_detect(pt, gt, P, d_frames, P.out.data_ptr(), **kw) == pt._lib.PDOG_E_ARG
            assert b"rank 1" in pt.lib().pdog_last_error()
        gt.sync()
        assert untouched(P)                                        # nothing ran
        # a null `out` is refused before GroupStart …
        assert raw_detect(pt, gt, P, d_frames, 0) == pt._lib.PDOG_E_ARG
        gt.sync()
        assert untouched(P)
        # … so the next call does not find a group left open (its gather would not be issued)
        assert raw_detect(pt, gt, P, d_frames, P.out.data_ptr()) == 0
        gt.sync()
        verify(P)
        # an empty shard may come with null pointers: one window, ranks 1 and 2 own nothing
        Q = upload(plan(pt, sc, oracle, ranks, 1, True))
        assert Q.n == [1, 0, 0]
        torch.cuda.synchronize()
        assert raw_detect(pt, gt, Q, d_frames, Q.out.data_ptr(), null_frames=(1, 2), null_guesses=(1, 2)) == 0
        gt.sync()
        verify(Q)
    finally:
        gt.close()


def test_a_rank_whose_batch_is_refused_after_rank_0_has_launched(pt, oracle, sc, d_frames):
    """n_frames[1] = 0 is what pdog_detect_batch itself refuses (check_stack), for rank 1 only: rank 0's kernels are queued by
    then.  The call returns that code, no gather is issued (out keeps its preset), sync is clean, the group goes on working."""
    import torch
    ranks = 3
    gt = _group(pt, sc, ranks)
    try:
        P = upload(plan(pt, sc, oracle, ranks, 10, True))
        torch.cuda.synchronize()
        nf = [d_frames[r].shape[0] for r in range(ranks)]
        nf[1] = 0
        assert raw_detect(pt, gt, P, d_frames, P.out.data_ptr(), n_frames=nf) == pt._lib.PDOG_E_ARG
        assert b"pdog_detect_batch: bad size/stride" in pt.lib().pdog_last_error()
        gt.sync()
        assert untouched(P)
        assert torch.cuda.current_device() == 0
        for n_total in (10, 11):
            Q = upload(plan(pt, sc, oracle, ranks, n_total, True, salt=6))
            torch.cuda.synchronize()
            gt.detect(d_frames[:ranks], Q.d_g, n_total, Q.out, frame_index=Q.d_fi)
            gt.sync()
            verify(Q)
    finally:
        gt.close()


# ---- e. the layer above ----
def test_group_tracker_local_handle(pt, oracle, sc, d_frames):
    import torch
    gt = _group(pt, sc, 3)
    assert gt.size() == 3 and gt.devices == [0, 0, 0]
    assert [gt.shard(11, r) for r in range(3)] == [(0, 4), (4, 8), (8, 11)] and gt.shard(2, 2) == (2, 2)
    for r in range(3):
        i = gt.info(r)
        assert (i.frame_h, i.frame_w, i.win_h, i.win_w, i.kernel_len, i.fill) == (sc.h, sc.w, 21, 21, 29, sc.fill)
    streams = [gt.stream(r) for r in range(3)]
    assert all(streams) and len(set(streams)) == 3                 # a stream of its own per rank, none the null stream
    gt.reserve(4098)
    gt.reserve(2)                                                  # (a rank without a window reserves for one)
    P = upload(plan(pt, sc, oracle, 3, 10, True))
    torch.cuda.synchronize()
    for wrong in (d_frames[:2], d_frames[:4]):
        with pytest.raises(ValueError):
            gt.detect(wrong, P.d_g, 10, P.out, frame_index=P.d_fi)
    with pytest.raises(ValueError):
        gt.detect(d_frames[:3], P.d_g[:2], 10, P.out, frame_index=P.d_fi)
    with pytest.raises(ValueError):
        gt.detect(d_frames[:3], P.d_g, 10, P.out, frame_index=P.d_fi[:2])
    assert untouched(P)
    for _ in range(3):                                             # never synced: close() drains every rank first
        gt.detect(d_frames[:3], P.d_g, 10, P.out, frame_index=P.d_fi)
    gt.close()
    torch.cuda.synchronize()
    verify(P)
    with pytest.raises(pt.PdogError):                              # 1 … 64 ranks, an ordinal that exists
        pt.GroupTracker.local(0, sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)
    with pytest.raises(pt.PdogError):
        pt.GroupTracker.local(65, sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill)
    with pytest.raises(pt.PdogError) as e:
        pt.GroupTracker.local(2, sc.h, sc.w, sc.tw, sc.ws, sc.darker, sc.fill, device=torch.cuda.device_count())
    assert e.value.code == pt._lib.PDOG_E_NODEV
