"""How the workgroups of the pre-pass meet (csrc/dog_prune.hpp, the publish block; csrc/dog_prune_publish.hpp): by default one
relaxed atomic per workgroup on a packed word (arrivals, jobs appended, pairs kept), from which the batch's last arriver
takes the list's length and the batch's kept pairs; with `fenced_publish` = 1 (and for batches whose counts do not fit the
word's fields) per-workgroup counts and an acquire-release arrival.  Nothing the caller sees may differ between the two, or
between either and the dense path.  Everything is decided by exact equality, with the helpers of
tests/test_gpu_prune_compact.py and tests/test_gpu_prune_lengths.py; the packing itself is tests/test_prune_publish_cpu.py's.

Frames of 300 × 400, l = 65, windows of 65 × 101 (two strips) and 129 × 197 (three strips and five remainder columns).  The
37 windows of a geometry differ in their job count: a disc that one strip alone keeps (the first strip, or the last), a disc
in each strip (the later ones a little fainter: no tie), and noise-only windows that keep everything — asserted on the
restatement's hulls (tests/prune_restatement.py) before anything runs on the GPU.

test_publish_forms_agree: the same five calls — batches of 1, 9, 37, 9 and 1 windows — on ONE tracker per build, for the
builds default, `fenced_publish` = 1 and `no_prune` = 1, exact mode on, the roll variant pinned.  After every call: positions
equal in all three builds and equal to the dense Float64 oracle's, merged maxima bit-equal, as many windows re-evaluated, and
prune_counts() the restatement's cumulative (kept, total) in both pruned builds ((0, 0) in the dense one).  The batch sizes
make the last arriver's sums (the list's header, the kept pairs) those of one window, of a few, and of many workgroups in
flight at once, and the word must be zero again for the next call.  That every call is a pruned one is a property of the
inputs: PrunePolicy (csrc/pdog_policy.hpp), restated, is fed the restatement's counts and must say so.

test_host_word_puts_the_policy_to_sleep: what the last arriver leaves in Mailbox::prune_pub is read by the host's policy and
by nothing else.  On a fresh tracker a batch of windows that keep more than kPruneBreakEvenPct of their pairs (by the
restatement, asserted first) must send the next, prunable batch down the dense path: that call counts nothing, in both
publish forms.

(`no_roll_map` in every build, as in tests/test_gpu_prune_lengths.py's interleaved test: the noise-only windows are near-ties
that exact mode re-evaluates, MapPolicy would answer with the response map, and a launch that writes the map cannot prune.)
Measured on an MI355X: the file's 4 tests together 3.2 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_restatement as pr  # noqa: E402
from test_gpu_prune_compact import FILL, _Set, _frame, _rad  # noqa: E402
from test_gpu_prune_lengths import _PrunePolicy, _Tracker, _bits  # noqa: E402

pytestmark = pytest.mark.gpu

L, FH, FW, NWIN = 65, 300, 400, 37
SHAPES = ((65, 101), (129, 197))
CALLS = ((0, 1), (0, 9), (0, 37), (5, 14), (36, 37))            # batches of 1, 9, 37, 9 and 1 windows
KINDS = ("first", "last", "each", "first", "all", "last", "first", "last", "first")   # window k is of kind KINDS[k % 9]
BUILDS = (("default", {}), ("fenced_publish", {"fenced_publish": 1}), ("no_prune", {"no_prune": 1}))


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _noise(f, a, rng):
    return np.clip(f.astype(np.int16) + rng.integers(-a, a + 1, f.shape), 0, 255).astype(np.uint8)


def _window(ws, k, kind, rng):
    """(frame, guess) of window k: discs at window columns that the first strip alone, the last strip alone or every strip
    reads (a strip reads its 64 columns and l ÷ 2 to either side), or noise alone."""
    rad, (n1, n2) = _rad(L), ws
    g = (150 + k % 5 - 2, 200 + (3 * k) % 7 - 3)
    oy, ox = g[0] - 1 - n1 // 2, g[1] - 1 - n2 // 2             # frame row / column of window pixel (0, 0)
    wy = n1 // 2 + (7 * k) % 21 - 10
    if kind == "all":
        return _noise(np.full((FH, FW), FILL, np.uint8), 3, rng), g
    starts = [c0 for c0, w in pr.slots(n2) if w > 1]
    if kind == "first":
        cols = [(2, 0)]
    elif kind == "last":
        cols = [(min(starts[-1] + 61, n2 - 3), 0)]
    else:                                                       # the middle of the columns each strip reads alone, or nearly
        mids = [2] + [c0 + 31 for c0 in starts[1:-1]] + [min(starts[-1] + 61, n2 - 3)]
        cols = [(c, 10 * i) for i, c in enumerate(mids)]
    f = np.full((FH, FW), FILL, np.uint8)
    for i, (c, value) in enumerate(cols):
        f = np.where(_frame(FH, FW, [(oy + wy + (5 * i) % 11 - 5, ox + c)], rad) == 0, value, f).astype(np.uint8)
    return _noise(f, 1, rng), g


_SETS = {}


def _set(oracle, ws):
    if ws not in _SETS:
        rng = np.random.default_rng([L, *ws])
        wins = [_window(ws, k, KINDS[k % 9], rng) for k in range(NWIN)]
        _SETS[ws] = _Set(oracle, L, ws, FH, FW, [f for f, _ in wins], [g for _, g in wins])
    return _SETS[ws]


def _jobs(st, w):
    return sum(bb > ba for ba, bb in st.pps[w]["hull"][:st.nstrips])


def _inputs_are_what_they_claim(st):
    """The restatement's view of the 37 windows: job counts by kind, and a kept share per call that keeps PrunePolicy awake."""
    for w in range(NWIN):
        kind, hull, (kept, total) = KINDS[w % 9], st.pps[w]["hull"], st.pairs[w]
        strips = [bb > ba for ba, bb in hull[:st.nstrips]]
        if kind == "first":
            assert strips == [True] + [False] * (st.nstrips - 1), (w, hull)
        elif kind == "last":
            assert strips == [False] * (st.nstrips - 1) + [True], (w, hull)
        elif kind == "each":
            assert all(strips), (w, hull)
        else:
            assert kept == total, (w, hull)
    assert {_jobs(st, w) for w in range(NWIN)} >= {1, st.nstrips}
    policy = _PrunePolicy()
    kept = total = 0
    for a, b in CALLS:
        assert policy.decide(kept, total), ((a, b), kept, total)
        k, t = st.want(a, b)
        assert 0 < k < t
        kept, total = kept + k, total + t
    return policy


@pytest.mark.parametrize("ws", SHAPES, ids=("65x101", "129x197"))
def test_publish_forms_agree(pt, oracle, ws):
    st = _set(oracle, ws)
    assert st.nstrips == (2 if ws == (65, 101) else 3) and len(st.pps[0]["hull"]) == st.nstrips + (0 if ws == (65, 101) else 5)
    _inputs_are_what_they_claim(st)
    trackers = {name: _Tracker(*st.args(pt), 1, no_roll_map=1, **tuning) for name, tuning in BUILDS}
    try:
        kept = total = 0
        for i, (a, b) in enumerate(CALLS):
            frames, guesses = st.frames[a:b], st.guesses[a:b]
            k, t = st.want(a, b)
            kept, total = kept + k, total + t
            runs = {name: trackers[name].run(frames, guesses) for name, _ in BUILDS}
            pos_d, max_d, ref_d, counts_d = runs["no_prune"]
            assert counts_d == (0, 0), (i, counts_d)
            assert np.array_equal(pos_d, st.ref[a:b]), (i, np.argwhere(pos_d != st.ref[a:b])[:4])
            for name in ("default", "fenced_publish"):
                pos, mx, refined, counts = runs[name]
                print(f"prune publish {ws} call {i} [{a}:{b}] {name}: jobs {sum(_jobs(st, w) for w in range(a, b))}, counts {counts}, "
                      f"the restatement {(kept, total)}; refined {refined} / {ref_d}")
                assert counts == (kept, total), (i, name, counts, (kept, total))
                assert np.array_equal(pos, st.ref[a:b]), (i, name, np.argwhere(pos != st.ref[a:b])[:4])
                assert np.array_equal(pos, pos_d), (i, name)
                assert np.array_equal(_bits(mx), _bits(max_d)), (i, name, np.argwhere(_bits(mx) != _bits(max_d))[:4])
                assert refined == ref_d, (i, name, refined, ref_d)
    finally:
        for t in trackers.values():
            t.close()


@pytest.mark.parametrize("fenced", (0, 1), ids=("default", "fenced_publish"))
def test_host_word_puts_the_policy_to_sleep(pt, oracle, fenced):
    st = _set(oracle, SHAPES[0])
    full = [w for w in range(NWIN) if KINDS[w % 9] == "all"]
    prunable = [w for w in range(NWIN) if KINDS[w % 9] == "first"][:len(full)]
    # the restatement alone, before the kernel is consulted: the first batch keeps more than the break-even share, the second would prune
    policy = _PrunePolicy()
    k1, t1 = (sum(st.pairs[w][i] for w in full) for i in (0, 1))
    k2, t2 = (sum(st.pairs[w][i] for w in prunable) for i in (0, 1))
    assert len(full) == len(prunable) == 4 and k1 * 100 > t1 * (100 - policy.pre_pct) and k2 * 100 < t2 * (100 - policy.pre_pct), ((k1, t1), (k2, t2))
    assert policy.decide(0, 0) and not policy.decide(k1, t1)    # the call after the first batch runs dense
    t = _Tracker(*st.args(pt), 1, no_roll_map=1, fenced_publish=fenced)
    try:
        pos, _, _, counts = t.run(st.frames[full], st.guesses[full])
        assert counts == (k1, t1), (counts, (k1, t1))
        assert np.array_equal(pos, st.ref[full])
        pos, _, _, counts = t.run(st.frames[prunable], st.guesses[prunable])
        print(f"prune publish host word fenced={fenced}: after the full batch {(k1, t1)}, after the prunable one {counts}")
        assert counts == (k1, t1), (counts, (k1, t1))           # the policy sleeps: the prunable batch counted nothing
        assert np.array_equal(pos, st.ref[prunable])
    finally:
        t.close()
