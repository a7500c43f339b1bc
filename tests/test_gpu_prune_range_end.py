"""The END of a kept range in the PRUNE instances of the roll kernel (csrc/dog_roll.hpp, roll_col_body ENTRY; the rule is
csrc/dog_roll_range.hpp's): the last sub-chunks of a range enter their column-pass body at the first tap block that still
feeds an emitted output, rounded down to the entry step (4 blocks up to l = 81, 8 above).  Everything is decided by exact
equality, with the helpers of tests/test_gpu_prune_compact.py and tests/test_gpu_prune_lengths.py.

What this file can and cannot show.  A wrong entry block shows on the GPU only if it lifts an output above the window's
maximum or within T of it (a lost term of the peak itself, or of a neighbour that then overtakes it), or if it breaks the
clipped case (the window's last rows, y_end = n1 − 1, with the peak inside the end zone).  The proof that EVERY emitted output
is whole is the static_assert of roll_end_covers / roll_end_meets_prologue per length and the two CPU tests
(tests/test_range_end_cpu.py: the rule against the row-tap pairs counted one by one; tests/test_range_end_emulation_cpu.py:
the slot machine in float32, bit for bit).

l = 17, 21, 65, 85 (NBODY = 3, 4, 9, 12 column-pass bodies; l = 21 is the length whose last sub-chunk emits rows past 8·bb,
l = 85 the first with two waves per SIMD) and l = 149 (NBODY = 20) with one batch of ten windows: the dense Float64 oracle of
its 485-row windows is the slow part, and ten one-strip windows cannot show twenty residues — that one property is asked of
the other four lengths only.  Windows are one strip wide, (24·NBODY + 5) × 63, in a frame that holds the centred tile with a
margin of four pixels; two of them hang over the frame's bottom.  One more case per length ≤ 85: two strips and a remainder
column, 101 × 129 (tests/test_gpu_prune_compact.py's batch B).

Before anything runs on the GPU the restatement's hulls (tests/prune_restatement.py) must show, with n = sc_hi − ba the
range's sub-chunks:
  * n mod NBODY takes every residue among the ranges the window's bottom does not cut off (l ≤ 85);
  * a range with n < roll_prologue_len + prune_tail — prologue and end overlap in one sub-chunk (a single small disc);
  * a range with n ≥ roll_prologue_len + prune_tail + NBODY — full bodies that are not entered late lie in between;
  * a range with sc_hi = nsub in a window with n1 mod 8 ≠ 0 whose oracle position lies in the window's last 8 rows — the
    clipped y_end = n1 − 1, the peak inside the end zone;
  * a range that ends within prune_tail sub-chunks of the bottom without reaching it;
  * a window that hangs over the frame's bottom with padding-only sub-chunks among the last prune_tail of its range —
    roll_col_zero where the entry would apply.
Then three configurations — default, `no_range_end` = 1, `no_prune` = 1 — with exact mode on and off: positions equal (exact
mode on: the dense Float64 oracle's), merged maxima bit-equal, as many windows re-evaluated, prune_counts() the restatement's
in both pruned runs.  test_toggle_on_one_tracker runs one batch through one tracker's batch calls with `no_range_end`
toggled between them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_restatement as pr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
from test_gpu_prune_compact import FILL, CH, _Set, _batch_b, _centred, _frame, _rad  # noqa: E402
from test_gpu_prune_lengths import _PrunePolicy, _Tracker, _bits, _once  # noqa: E402

pytestmark = pytest.mark.gpu

NBODY = {17: 3, 21: 4, 65: 9, 85: 12, 149: 20}


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _scenes(oracle, l):
    """One-strip windows of (24·NBODY + 5) × 63: a single disc, pairs of equal discs 8·m rows apart (the hull grows by a block
    per step), one long pair, a disc in the window's last rows, one a few blocks above them, and two windows that hang over
    the frame's bottom with a disc in the frame's last rows."""
    nbody, hw, rad = NBODY[l], l // 2, _rad(l)
    assert nbody == ps.roll_phases(l)
    ws = (24 * nbody + 5, 63)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    x, y0 = wj0 + 31, hw + rad + CH
    long_m, y_top = ps.roll_prologue_len(l) + nbody + 1, rad + 1            # the long pair starts in the window's first rows
    assert y_top + CH * long_m <= ws[0] - 2 - rad
    # (a few distances to spare: at some the hull's start moves too)
    steps = [m for m in range(1, nbody + 6) if y0 + CH * m <= ws[0] - 2 - rad] if l <= 85 else (1, 2, 3, 5)
    discs = [[(wi0 + y0, x)]]
    discs += [[(wi0 + y0, x), (wi0 + y0 + CH * m, x)] for m in steps]
    discs += [[(wi0 + y_top, x), (wi0 + y_top + CH * long_m, x)]]
    discs += [[(wi0 + ws[0] - 2, x)], [(wi0 + ws[0] - 2 - CH * (pr.tail(l) // 2 + 1), x)]]
    guesses = [g] * len(discs)
    for hang in (hw + 2 * CH, hw + 5 * CH):                   # window rows below the frame's last row
        discs.append([(fh - 2 - rad, x)])
        guesses.append((g[0] + 4 + hang, g[1]))
    frames = [_frame(fh, fw, d, rad) for d in discs]
    # a single SMALL disc (radius 1) in the last rows of the tile's first sub-chunk, which only output block 0 reads: at the
    # short lengths the one scene whose hull is a single block, so that prologue and end meet in one sub-chunk (l = 17, 21:
    # n < roll_prologue_len + prune_tail means n = prune_tail + 1; from l = 65 on the disc in the window's last rows gives the form)
    if l <= 21:
        frames.append(_frame(fh, fw, [(wi0 - hw + CH - 2, x)], 1))
        guesses.append(g)
    return _Set(oracle, l, ws, fh, fw, frames, guesses)


def _forms(st):
    """The properties of the docstring, read off the restatement's hulls: {name: [window, …]} and the residues of n."""
    l, nbody, tail, npro = st.l, NBODY[st.l], pr.tail(st.l), ps.roll_prologue_len(st.l)
    hw, n1 = l // 2, st.ws[0]
    found = {k: [] for k in ("overlap", "long", "clipped peak", "near bottom", "padding in the end zone")}
    residues = set()
    for w, (pp, g, ref) in enumerate(zip(st.pps, st.guesses, st.ref)):
        assert len(pp["hull"]) == 1
        (ba, bb), nsub = pp["hull"][0], pp["nsub"]
        assert bb > ba, (l, w)
        sc_hi = min(bb + tail, nsub)
        n = sc_hi - ba
        cut = bb + tail >= nsub
        if not cut:
            residues.add(n % nbody)
        if n < npro + tail:
            found["overlap"].append(w)
        if n >= npro + tail + nbody:
            found["long"].append(w)
        # the oracle's 1-based frame position → window row
        yw = int(ref[0]) - 1 - (int(g[0]) - st.radii[0] - 1)
        if cut and n1 % CH != 0 and n1 - CH <= yw < n1:
            found["clipped peak"].append(w)
        if not cut and sc_hi >= nsub - tail:
            found["near bottom"].append(w)
        ti0 = int(g[0]) - st.radii[0] - 1 - hw
        pad_bot = max(0, (st.fh - ti0 + CH - 1) >> 3)
        if pp["dc"] == FILL and max(ba, sc_hi - tail) <= pad_bot < sc_hi:
            found["padding in the end zone"].append(w)
    return found, residues


def _three_ways(pt, st, what):
    want = st.want()
    assert 0 < want[0] < want[1], (what, want)
    res = {}
    for exact in (1, 0):
        runs = {name: _once(*st.args(pt), st.frames, st.guesses, exact, **tuning)
                for name, tuning in (("default", {}), ("no_range_end", {"no_range_end": 1}), ("no_prune", {"no_prune": 1}))}
        pos_d, max_d, ref_d, counts_d = runs["no_prune"]
        assert counts_d == (0, 0)
        if exact:
            assert np.array_equal(pos_d, st.ref), (what, np.argwhere(pos_d != st.ref)[:4])
        for name in ("default", "no_range_end"):
            pos, mx, refined, counts = runs[name]
            print(f"range end {what} l={st.l} exact={exact} {name}: kept {counts[0]} of {counts[1]}, the restatement {want[0]} of {want[1]}; refined {refined} / {ref_d}")
            assert np.array_equal(pos, pos_d), (what, name, exact, np.argwhere(pos != pos_d)[:4])
            if exact:
                assert np.array_equal(pos, st.ref), (what, name, np.argwhere(pos != st.ref)[:4])
            assert np.array_equal(_bits(mx), _bits(max_d)), (what, name, exact, np.argwhere(_bits(mx) != _bits(max_d))[:4])
            assert refined == ref_d, (what, name, exact)
            assert counts == want, (what, name, exact, counts, want)
        res[exact] = runs["default"][1]
    assert np.array_equal(_bits(res[0]), _bits(res[1]))


_SETS = {}


def _set(oracle, l):
    if l not in _SETS:
        _SETS[l] = _scenes(oracle, l)
    return _SETS[l]


@pytest.mark.parametrize("l", (17, 21, 65, 85, 149))
def test_range_ends_of_every_form(pt, oracle, l):
    st = _set(oracle, l)
    found, residues = _forms(st)
    assert st.nstrips == 1 and st.ws[0] % CH == 5 and len(st.frames) <= (10 if l == 149 else NBODY[l] + 12)
    assert all(found.values()), (l, found, [pp["hull"] for pp in st.pps])
    if l <= 85:
        assert residues == set(range(NBODY[l])), (l, residues, [pp["hull"] for pp in st.pps])
    _three_ways(pt, st, "one strip")


@pytest.mark.parametrize("l", (17, 21, 65, 85))
def test_two_strips_and_a_remainder_column(pt, oracle, l):
    st = _batch_b(oracle, l)
    assert st.nstrips == 2 and st.ws == (101, 129) and all(len(pp["hull"]) == 3 for pp in st.pps)
    _three_ways(pt, st, "two strips")


def test_toggle_on_one_tracker(pt, oracle):
    st = _set(oracle, 65)
    nw = 8                                                   # the single disc and the first pairs: short ranges, a small kept share
    frames, guesses, ref, want = st.frames[:nw], st.guesses[:nw], st.ref[:nw], st.want(0, nw)
    dense = _once(*st.args(pt), frames, guesses, 1, no_prune=1)
    assert np.array_equal(dense[0], ref)
    policy = _PrunePolicy()                                  # (a batch that keeps too much sends the tracker's next batches down the dense path)
    # (the windows with two equal discs are near-ties that exact mode re-evaluates; MapPolicy would answer with the response map,
    # whose launches cannot prune: `no_roll_map`, as in tests/test_gpu_prune_lengths.py's interleaved test)
    t = _Tracker(*st.args(pt), 1, no_roll_map=1)
    try:
        kept = total = 0
        for i, off in enumerate((0, 1, 0, 1)):
            assert policy.decide(kept, total), (i, want)     # a property of the inputs: every call is a pruned one
            t.bt.set_tuning("no_range_end", off)
            pos, mx, _, counts = t.run(frames, guesses)
            kept, total = kept + want[0], total + want[1]
            assert counts == (kept, total), (i, counts, (kept, total))
            assert np.array_equal(pos, ref), (i, off, np.argwhere(pos != ref)[:4])
            assert np.array_equal(_bits(mx), _bits(dense[1])), (i, off)
    finally:
        t.close()
