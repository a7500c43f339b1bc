"""The pruned roll batch path with the pre-pass's JOB LIST (csrc/dog_prune.hpp, "the job list"; the PRUNE instances of
csrc/dog_roll.hpp): the pre-pass appends a window's kept strips to a compact list, leaves the finished partial of every strip
with an empty hull itself, and hands the window's DC level on (to the strips in their list entry, to dog_thin_kernel in its
range word); a strip numbers its sub-chunks from the first one of its kept range, so the shortened prologue bodies serve every
range.  Everything is decided by exact equality, as in tests/test_gpu_prune_lengths.py, whose helpers this file uses.

test_range_starts_and_lengths, l = 17, 65, 85, 149 (3, 9, 12, 20 column-pass bodies, NBODY = roll_slots(l) / 8).  A window's
width is 2·(w ÷ 2) + 1, always odd, so "one strip, no remainder column" is 63 columns here and "strips plus a remainder
column" 129.  Batch A, windows of (24·NBODY + 5) × 63: a disc stepped down by 8 rows per window (the hull's first block ba
takes every residue mod NBODY), a disc with a second equal one at a growing distance (bb − ba takes every residue), a disc in
the first rows (ba = 0) and one in the last (bb = the last block of a height that is no multiple of 8).  Batch B, windows of
101 × 129: discs in one strip, across the strip boundary, on the remainder column, in the first and the last rows.  The
restatement's hulls (tests/prune_restatement.py) must show all of that before anything runs on the GPU.  Pruning on against
`no_prune`, exact mode on and off: positions equal (exact mode on: the dense Float64 oracle's too), merged maxima bit-equal,
as many windows re-evaluated, prune_counts() the restatement's.

test_padding_inside_a_kept_range: windows hanging over the frame's top and bottom whose kept range holds padding-only
sub-chunks (asserted from the hull and the tile's position): roll_col_zero under the relative phase.
test_dc_level_per_job: windows whose DC level is the fill beside windows more than 8 levels away from it, in one batch.
test_one_tracker_many_batches: the list's count and stale entries — the same batch three times, a larger one, a smaller one,
`no_prune` and back, on one tracker.
test_list_lengths: batches of 1, 3 and 9 windows (list lengths that are no multiple of 8) and a batch whose every strip is kept.
Measured on an MI355X: the file's 9 tests together 4.1 s, most of it the dense oracle of l = 149 (47 windows of 485 × 63)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
from test_gpu_prune_lengths import _Tracker, _bits, _once  # noqa: E402

pytestmark = pytest.mark.gpu

FILL, CH = 128, 8


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _rad(l):
    return max(2, int(ps.tw_for_kernel_len(l)) // 2)


def _frame(fh, fw, discs, rad, background=FILL, value=0):
    """discs: 0-based (frame row, frame column) centres."""
    f = np.full((fh, fw), background, np.uint8)
    ii, jj = np.ogrid[:fh, :fw]
    for cy, cx in discs:
        f[(ii - cy) ** 2 + (jj - cx) ** 2 <= rad * rad] = value
    return f


class _Set:
    """Windows of one size in one frame geometry: the frames, the oracle's positions, the restatement's pre-passes."""

    def __init__(self, oracle, l, ws, fh, fw, frames, guesses, fill=FILL, darker=True):
        self.l, self.ws, self.fh, self.fw, self.fill, self.darker = l, ws, fh, fw, fill, darker
        self.frames, self.guesses = np.stack(frames), np.array(guesses, np.int32)
        self.radii = (ws[0] // 2, ws[1] // 2)
        tw = ps.tw_for_kernel_len(l)
        sg = oracle.sigma(tw)
        assert oracle.kernel_len(sg) == l
        self.ref = oracle.detect_batch_par(self.frames, fill, oracle.dog_kernel(sg, darker), sg, darker, self.radii, self.guesses, separable=False)
        self.pps = [pr.prepass(fr.window_tile(f, fill, l, self.radii, g), fill, tw, darker) for f, g in zip(self.frames, self.guesses)]
        self.pairs = [pr.kept_pairs(pp, l) for pp in self.pps]
        self.nstrips = sum(1 for _, w in self.pps[0]["slots"] if w > 1)

    def want(self, a=0, b=None):
        p = self.pairs[a:b]
        return sum(k for k, _ in p), sum(t for _, t in p)

    def args(self, pt):
        return (pt, self.fh, self.fw, self.l, self.ws, self.darker, self.fill)


def _centred(l, ws, margin=4):
    """A frame that holds the whole tile of a window at its centre: (fh, fw, guess, frame row / column of window pixel (0, 0))."""
    n1, n2 = ws
    fh, fw = n1 + l - 1 + 2 * margin, n2 + l - 1 + 2 * margin
    g = (fh // 2 + 1, fw // 2 + 1)
    return fh, fw, g, (g[0] - n1 // 2 - 1, g[1] - n2 // 2 - 1)


def _compare(pt, st, what):
    """Pruned against `no_prune`, exact mode on and off."""
    want = st.want()
    assert 0 < want[0] < want[1], (what, want)
    res = {}
    for exact in (1, 0):
        pos_p, max_p, ref_p, counts_p = _once(*st.args(pt), st.frames, st.guesses, exact, no_prune=0)
        pos_d, max_d, ref_d, counts_d = _once(*st.args(pt), st.frames, st.guesses, exact, no_prune=1)
        print(f"prune compact {what} l={st.l} exact={exact}: kept {counts_p[0]} of {counts_p[1]}, the restatement {want[0]} of {want[1]}; refined {ref_p} / {ref_d}")
        assert np.array_equal(pos_p, pos_d), (what, exact, np.argwhere(pos_p != pos_d)[:4])
        if exact:
            assert np.array_equal(pos_d, st.ref), (what, np.argwhere(pos_d != st.ref)[:4])
            assert np.array_equal(pos_p, st.ref), (what, np.argwhere(pos_p != st.ref)[:4])
        assert np.array_equal(_bits(max_p), _bits(max_d)), (what, exact, np.argwhere(_bits(max_p) != _bits(max_d))[:4])
        assert ref_p == ref_d, (what, exact)
        assert counts_d == (0, 0) and counts_p == want, (what, exact, counts_p, want)
        assert counts_p[0] < counts_p[1]
        res[exact] = max_p
    assert np.array_equal(_bits(res[0]), _bits(res[1]))


# ---- every start phase and every range length of every body count ----
def _batch_a(oracle, l):
    nbody, hw, rad = ps.roll_phases(l), l // 2, _rad(l)
    ws = (24 * nbody + 5, 63)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    x = wj0 + 31
    step = [[(wi0 + hw + rad + CH * k, x)] for k in range(nbody)]                                           # ba: one block more per window
    # bb − ba: a block more per window, but for the few distances at which the hull's start moves too: five distances to spare
    y0 = hw + rad + CH
    pair = [[(wi0 + y0, x), (wi0 + y0 + CH * m, x)] for m in range(1, nbody + 6) if y0 + CH * m <= ws[0] - 2]
    ends = [[(wi0 + 2, x)], [(wi0 + ws[0] - 2, x)]]
    discs = step + pair + ends
    assert len(discs) <= 64
    return _Set(oracle, l, ws, fh, fw, [_frame(fh, fw, d, rad) for d in discs], [g] * len(discs))


def _batch_b(oracle, l):
    rad = _rad(l)
    ws = (101, 129)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    discs = [[(wi0 + 50, wj0 + 31)], [(wi0 + 40, wj0 + 64)], [(wi0 + 60, wj0 + 128)], [(wi0 + 50, wj0 + 96)],
             [(wi0 + 1, wj0 + 20)], [(wi0 + 99, wj0 + 120)]]
    return _Set(oracle, l, ws, fh, fw, [_frame(fh, fw, d, rad) for d in discs], [g] * len(discs))


@pytest.mark.parametrize("l", (17, 65, 85, 149))
def test_range_starts_and_lengths(pt, oracle, l):
    nbody = ps.roll_phases(l)
    assert nbody == {17: 3, 65: 9, 85: 12, 149: 20}[l]
    a = _batch_a(oracle, l)
    hulls = [pp["hull"][0] for pp in a.pps]
    nblk = a.pps[0]["nblk"]
    assert a.nstrips == 1 and len(a.pps[0]["hull"]) == 1 and nblk >= 3 * nbody and a.ws[0] % CH != 0
    assert all(bb > ba for ba, bb in hulls), hulls
    assert {ba % nbody for ba, _ in hulls} == set(range(nbody)), (l, hulls)
    assert {(bb - ba) % nbody for ba, bb in hulls} == set(range(nbody)), (l, hulls)
    assert any(ba == 0 for ba, _ in hulls) and any(bb == nblk for _, bb in hulls), (l, hulls)
    assert any(ba >= ps.roll_prologue_len(l) for ba, _ in hulls)
    _compare(pt, a, "A")
    b = _batch_b(oracle, l)
    hb = [pp["hull"] for pp in b.pps]
    assert b.nstrips == 2 and all(len(h) == 3 for h in hb)
    kept = [[bb > ba for ba, bb in h] for h in hb]
    if l <= 85:   # (a strip of l = 149 reads 212 of the tile's 277 columns: a disc of radius 28 is in sight of both)
        assert any(k[0] and not k[1] for k in kept) and any(k[1] and not k[0] for k in kept), hb # an empty strip beside a kept one, either way
    assert any(k[0] and k[1] for k in kept), hb
    assert any(k[2] for k in kept) and any(not k[2] for k in kept), hb                            # the remainder column kept and empty
    _compare(pt, b, "B")


# ---- padding-only sub-chunks inside a kept range ----
@pytest.mark.parametrize("l", (17, 65))
def test_padding_inside_a_kept_range(pt, oracle, l):
    hw, rad, fh, fw, ws = l // 2, _rad(l), 200, 300, (133, 63)
    top, bottom = (3, 150), (fh - 2, 150)               # guesses (1-based): the window hangs 60 rows and more over the edge
    frames, guesses = [], []
    for g, rows in ((top, (2, 9, 20)), (bottom, (fh - 3, fh - 10, fh - 24))):
        for r in rows:
            frames.append(_frame(fh, fw, [(r, g[1] - 1 + (r % 5) - 2)], rad))
            guesses.append(g)
    st = _Set(oracle, l, ws, fh, fw, frames, guesses)
    above = below = 0
    for g, pp in zip(st.guesses, st.pps):
        assert pp["dc"] == FILL                          # the skip needs the DC level at the fill
        (ba, bb), nsub = pp["hull"][0], pp["nsub"]
        assert bb > ba
        sc_hi = min(nsub, bb + pr.tail(l))
        ti0 = int(g[0]) - st.radii[0] - 1 - hw
        pad_top, pad_bot = max(0, -ti0) // CH, max(0, (fh - ti0 + CH - 1) >> 3)
        above += ba < min(pad_top, sc_hi)                # a padding-only sub-chunk inside [ba, sc_hi)
        below += pad_bot < sc_hi and pad_bot >= ba
    assert above >= 2 and below >= 2, (above, below)
    _compare(pt, st, "padding")


# ---- the DC level is the job's ----
def test_dc_level_per_job(pt, oracle):
    l, ws = 65, (101, 129)
    rad = _rad(l)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    frames = []
    for k, background in enumerate((FILL, 90, FILL, 200, 60, FILL)):
        frames.append(_frame(fh, fw, [(wi0 + 20 + 12 * k, wj0 + (31, 128, 70)[k % 3])], rad, background=background, value=0 if background > 30 else 255))
    st = _Set(oracle, l, ws, fh, fw, frames, [g] * len(frames))
    dcs = [pp["dc"] for pp in st.pps]
    assert dcs.count(FILL) == 3 and sum(abs(d - FILL) > 8 for d in dcs) == 3 and len(set(dcs)) == 4, dcs
    assert any(pp["hull"][2][1] > pp["hull"][2][0] and pp["dc"] != FILL for pp in st.pps)          # a kept remainder column away from the fill
    _compare(pt, st, "dc")


# ---- one tracker: the list's count, stale entries ----
def _mixed(oracle, n):
    l, ws = 65, (101, 129)
    rad = _rad(l)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    cols = (31, 64, 128, 96, 10, 120, 50)
    discs = [[(wi0 + 8 + (11 * k) % 90, wj0 + cols[k % len(cols)])] for k in range(n)]
    return _Set(oracle, l, ws, fh, fw, [_frame(fh, fw, d, rad) for d in discs], [g] * n)


def test_one_tracker_many_batches(pt, oracle):
    st = _mixed(oracle, 20)
    full_pos, full_max, _, full_counts = _once(*st.args(pt), st.frames, st.guesses, 1, no_prune=0)
    assert np.array_equal(full_pos, st.ref) and full_counts == st.want()
    t = _Tracker(*st.args(pt), 1)
    try:
        kept = total = 0
        first = None
        calls = [(0, 8, 0), (0, 8, 0), (0, 8, 0), (0, 20, 0), (0, 5, 0), (0, 8, 1), (0, 8, 0), (3, 20, 0), (0, 1, 0)]
        for i, (a, b, dense) in enumerate(calls):
            t.bt.set_tuning("no_prune", dense)
            pos, mx, _, counts = t.run(st.frames[a:b], st.guesses[a:b])
            if not dense:
                k, tt = st.want(a, b)
                kept, total = kept + k, total + tt
            assert counts == (kept, total), (i, counts, (kept, total))      # (a dense call counts nothing: the pruned ones did prune)
            if first is None:
                first = (pos.copy(), mx.copy())
                assert np.array_equal(pos, full_pos[:8]) and np.array_equal(_bits(mx), _bits(full_max[:8]))
            if b <= 8:
                assert np.array_equal(pos, first[0][a:b]) and np.array_equal(_bits(mx), _bits(first[1][a:b])), i
            assert np.array_equal(pos, full_pos[a:b]), (i, np.argwhere(pos != full_pos[a:b])[:4])
            assert np.array_equal(_bits(mx), _bits(full_max[a:b])), i
    finally:
        t.close()


# ---- list lengths that are no multiple of 8; every strip kept ----
def test_list_lengths(pt, oracle):
    st = _mixed(oracle, 9)
    dense_pos, dense_max, _, _ = _once(*st.args(pt), st.frames, st.guesses, 1, no_prune=1)
    assert np.array_equal(dense_pos, st.ref)
    for n in (1, 3, 9):
        jobs = sum(bb > ba for pp in st.pps[:n] for ba, bb in pp["hull"][:2])
        pos, mx, _, counts = _once(*st.args(pt), st.frames[:n], st.guesses[:n], 1, no_prune=0)
        print(f"prune compact list: {n} windows, {jobs} jobs")
        assert jobs % 8 != 0 and jobs < 2 * n
        assert counts == st.want(0, n) and np.array_equal(pos, st.ref[:n]) and np.array_equal(_bits(mx), _bits(dense_max[:n])), n
    # every strip kept: a disc in either strip of every window
    l, ws, rad = st.l, st.ws, _rad(st.l)
    fh, fw, g, (wi0, wj0) = _centred(l, ws)
    frames = [_frame(fh, fw, [(wi0 + 10 + 9 * k, wj0 + 20), (wi0 + 85 - 9 * k, wj0 + 110)], rad) for k in range(9)]
    full = _Set(oracle, l, ws, fh, fw, frames, [g] * 9)
    assert all(bb > ba for pp in full.pps for ba, bb in pp["hull"][:2])
    _compare(pt, full, "every strip kept")
