"""Chains over a frame table (pdog_detect_chains_indexed, BatchTracker.detect_chains_indexed, track_clips_indexed,
track_video): position for position equal to the plain chain over the materialised copy of the selected frames, and to
the restatement's loop over the oracle's functor (tests/video_restatement.py), on every kernel family that walks a table.
PARITY UNPINNED: the oracle is our restatement, see oracle/dog_oracle.c."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_restatement as vr  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 86399.999
SENT = -9


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- shared inputs: a stack with three dark discs on their own random walks, +-2 grey levels of noise ----
class Stack:
    def __init__(self, h, w, tw, nf, seed):
        rng = np.random.default_rng(seed)
        self.h, self.w, self.tw, self.nf = h, w, tw, nf
        rad = tw // 2
        frames = (128 + rng.integers(-2, 3, (nf, h, w))).astype(np.uint8)
        centre = np.array([[h // 4, w // 4], [h // 2, (2 * w) // 3], [(3 * h) // 4, w // 3]])
        self.pos = np.zeros((nf, 3, 2), int)
        yy, xx = np.ogrid[0:h, 0:w]
        for k in range(nf):
            centre = np.clip(centre + rng.integers(-3, 4, (3, 2)), rad + 2, [h - rad - 2, w - rad - 2])
            self.pos[k] = centre
            for ci, cj in centre:
                frames[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= rad * rad] = 5
        self.frames = frames
        self._dev = None
        self._memo = {}

    def dev(self):
        if self._dev is None:
            self._dev = _cuda(self.frames)
        return self._dev

    def fill(self, oracle):
        return oracle.mode_u8(self.frames[0])

    def chain(self, oracle, row, ws, start, first, fill=None):
        """The restatement's chain (vr.chain_indexed), functor applications memoised per (window, fill, frame, guess): the
        tables share most of them.  fill None: the mode of the stack's first frame."""
        K = self._memo.setdefault("K", oracle.dog_kernel(oracle.sigma(self.tw), True))
        fill = self.fill(oracle) if fill is None else int(fill)
        radii, out = (ws[0] // 2, ws[1] // 2), []
        for k in range(vr.row_len(row)):
            if k == 0 and first == 1:
                out.append((int(start[0]), int(start[1])))
                continue
            key = (ws, fill, int(row[k]), tuple(out[-1]) if k else (int(start[0]), int(start[1])))
            if key not in self._memo:
                self._memo[key] = tuple(oracle.detect(self.frames[key[2]], fill, K, radii, key[3]))
            out.append(self._memo[key])
        return out

    def starts(self, table):
        """Clip c follows disc c % 3: its start is that disc's place in the clip's first frame, a few pixels off."""
        return [tuple(int(v) for v in self.pos[max(int(row[0]), 0), c % 3] + (2, -3)) for c, row in enumerate(table)]


_STACKS = {}


def _stack(key):
    if key not in _STACKS:
        _STACKS[key] = {"small": lambda: Stack(96, 128, 10, 12, 5), "large": lambda: Stack(200, 240, 25, 16, 6)}[key]()
    return _STACKS[key]


def _tables(nf, ns):
    """The tables every path is held to, over a stack of nf = 2 ns frames."""
    assert nf == 2 * ns
    a = np.arange(ns)
    f3024 = [vr.fps_table(30, nf, s, BIG, 24)[:ns] for s in (0.0, 0.1)]          # drops: 0 1 3 4 5 6 ...
    f2430 = [vr.fps_table(24, nf, s, BIG, 30)[:ns] for s in (0.0, 0.2)]          # repeats: 0 1 1 2 3 4 ...
    assert all(len(r) == ns for r in f3024 + f2430) and f3024[0][:4] == [0, 1, 3, 4] and f2430[0][:4] == [0, 1, 1, 2]
    neg = [-1] * ns
    return {
        "identity": [a, a + ns],
        "reversed": [a[::-1] + ns, a[::-1]],
        "stride 2": [2 * a, 2 * a + 1],
        "30 to 24": f3024,
        "24 to 30": f2430,
        "two sharing": [a, a + 2],
        "three sharing": [a, a + 2, a + 4],
        "ragged": [list(a[:ns - 2]) + [-1, -1], neg, a + 3, [5] + neg[1:], a[::-1]],
    }


def _as_lists(t):
    return [[tuple(int(v) for v in r) for r in clip] for clip in t.cpu().numpy()]


def _check_table(pt, oracle, bt, st, ws, name, table, first):
    """One table, one value of first, on the tracker as the caller pinned it: the indexed chain against the restatement and
    against pdog_detect_chains over the gathered copy; rows at and beyond a clip's end keep the sentinel."""
    import torch
    table = np.asarray(table, np.int32).reshape(len(table), -1)
    nc, ns = table.shape
    starts = st.starts(table)
    d_starts = torch.tensor(starts, dtype=torch.int32).cuda()
    out = torch.full((nc, ns, 2), SENT, dtype=torch.int32).cuda()
    got = bt.detect_chains_indexed(st.dev(), table, d_starts, first=first, out=out)
    bt.sync()
    assert got is out
    got = _as_lists(out)
    lens = [vr.row_len(r) for r in table]
    for c in range(nc):
        want = st.chain(oracle, table[c], ws, starts[c], first)
        assert got[c][:lens[c]] == want, (name, first, c, got[c], want)
        assert all(p == (SENT, SENT) for p in got[c][lens[c]:]), (name, first, c)
        if first and lens[c]:
            assert got[c][0] == starts[c]
    # the materialised copy: a contiguous stack of the selected frames (an ended clip's tail reads frame 0, ignored below);
    # with first = 1 the plain chain starts at the second selected frame from the same start
    gathered = st.dev()[torch.from_numpy(np.maximum(table[:, first:], 0)).long().cuda()]
    if gathered.shape[1]:
        plain = _as_lists(bt.detect_chains(gathered, d_starts))
        bt.sync()
        for c in range(nc):
            assert got[c][first:lens[c]] == plain[c][:max(lens[c] - first, 0)], (name, first, c)


def _run_all_tables(pt, oracle, st, ws, ns, pin, clips=None):
    """Every table, first = 0 and 1, on a tracker that `pin` has set up; clips = 1 keeps only each table's first row."""
    bt = pt.BatchTracker(st.h, st.w, st.tw, ws, True, st.fill(oracle))
    try:
        pin(bt)
        for name, table in _tables(st.nf, ns).items():
            if clips is not None:
                table = table[:clips]
            for first in (0, 1):
                _check_table(pt, oracle, bt, st, ws, name, table, first)
    finally:
        bt.close()


# ---- 1. equality with the materialised copy and the restatement, per kernel family ----
@pytest.mark.parametrize("generic", (0, 1))
def test_fused_chain_over_a_table(pt, oracle, generic):
    """(a) one workgroup per clip, compile-time-length instance (l = 29) and the runtime-length one."""
    def pin(bt):
        bt.set_tuning("no_fused_c", generic)
        assert bt.info().kernel_len == 29 and bt.kernel_for_batch(1) == 300 and bt.kernel_for_batch(3) == 300
    _run_all_tables(pt, oracle, _stack("small"), (21, 21), 6, pin)


@pytest.mark.parametrize("ws", ((45, 45), (45, 97)))
def test_persistent_roll_chain_over_a_table(pt, oracle, ws):
    """(b) the l = 29 roll instance pinned: one strip, and two strips (a two-wave workgroup)."""
    def pin(bt):
        bt.set_variant(100 + 29)
        assert bt.info().variant == 129 and bt.kernel_for_batch(3) == 129 and bt.info().n_strips == (ws[1] + 63) // 64
    _run_all_tables(pt, oracle, _stack("small"), ws, 6, pin)


@pytest.mark.parametrize("clips", (1, 2))
def test_tiled_cooperative_chain_over_a_table(pt, oracle, clips):
    """(c) a 129 x 129 window (too large for one workgroup): one cooperative launch, one clip and two."""
    def pin(bt):
        assert bt.info().kernel_len == 65 and bt.kernel_for_batch(1) == 400 and bt.kernel_for_batch(2) == 400
    _run_all_tables(pt, oracle, _stack("large"), (129, 129), 8, pin, clips=clips)


@pytest.mark.parametrize("clips", (1, 2))
def test_fallback_launches_over_a_table(pt, oracle, clips):
    """(d) the tiled kernel pinned off: one clip is a launch per step whose frame the host names, two clips are the
    per-step batches whose frame index is a column of the table."""
    def pin(bt):
        bt.set_tuning("no_tiled", 1)
        assert bt.kernel_for_batch(1) != 400 and bt.kernel_for_batch(1) != 300
    _run_all_tables(pt, oracle, _stack("large"), (129, 129), 8, pin, clips=clips)


def test_per_step_batches_with_many_ragged_clips(pt, oracle):
    """The per-step batches again where they are cheap (the l = 29 ring kernel pinned), with every table at its full
    number of clips: ended clips ride along in the batches and must leave no trace."""
    def pin(bt):
        bt.set_variant(20)
        assert bt.info().variant == 20
    _run_all_tables(pt, oracle, _stack("small"), (21, 21), 6, pin)
    _run_all_tables(pt, oracle, _stack("small"), (21, 21), 6, pin, clips=1)


def test_a_table_of_one_step(pt, oracle):
    """n_steps = 1 is no chain for the kernels that walk a clip: it runs as launches, first = 0 and 1, on every pinning."""
    st = _stack("small")
    for pin in (lambda bt: None, lambda bt: bt.set_variant(129), lambda bt: bt.set_variant(20)):
        bt = pt.BatchTracker(st.h, st.w, st.tw, (21, 21), True, st.fill(oracle))
        pin(bt)
        for table in ([[3], [7], [-1]], [[4]]):
            for first in (0, 1):
                _check_table(pt, oracle, bt, st, (21, 21), "one step", table, first)
        bt.close()


# ---- 2. exact mode through the table ----
@pytest.mark.parametrize("kind", ("noise", "ties"))
@pytest.mark.parametrize("family", ("fused", "tiled"))
def test_exact_mode_refines_through_the_table(pt, oracle, family, kind):
    """The inline refinement re-reads the frame through the pointer derived from the table's entry.
    noise: frames of nothing but +-1 noise with EVERY window flagged (pdog_set_exact(t, 2): the whole restated computation on
    the device, every pixel of every window).  In the default mode such frames are flagged as well, but the window's own V
    withdraws the flags before anything is re-read — measured on 21 x 21 windows: 0 of 12 re-decided — so the
    default mode gets frames it must re-decide:
    ties: two equal specks on a flat background, at another place in every frame; their two peaks tie, the refinement decides
    for the first in column-major order (:59).
    Either way the indexed chain equals the chain over the materialised copy and the oracle's, and windows were refined."""
    import torch
    h, w, tw, ws, ns, sep = ((96, 128, 10, (45, 63), 6, 12) if family == "fused" else (200, 240, 25, (129, 129), 4, 28))
    nf = 2 * ns
    centre = [(h // 2 + f, w // 2 - 2 * f + (f % 3)) for f in range(nf)]     # (sep: both specks stay inside the window of a chain that follows the left one)
    if kind == "noise":
        frames = (128 + np.random.default_rng(17).integers(-1, 2, (nf, h, w))).astype(np.uint8)
    else:
        frames = np.full((nf, h, w), 128, np.uint8)
        for f, (ci, cj) in enumerate(centre):
            frames[f, ci - 1, cj - 1 - sep] = frames[f, ci - 1, cj - 1 + sep] = 118
    table = np.asarray(_tables(nf, ns)["30 to 24"], np.int32)
    starts = [tuple(int(v) for v in np.add(centre[table[0][0]], (1, 2))), tuple(int(v) for v in np.add(centre[table[1][0]], (-2, 1)))]
    # between two selected frames the specks move by at most 5 columns: the right one stays inside a window centred on the left one,
    # and 2 sep > 4 sigma keeps their two peaks apart
    assert 2 * sep + 5 <= ws[1] // 2 and sep > 2 * oracle.sigma(tw)
    d_starts = torch.tensor(starts, dtype=torch.int32).cuda()
    d_frames = _cuda(frames)
    bt = pt.BatchTracker(h, w, tw, ws, True, 128)
    assert bt.kernel_for_batch(2) == (300 if family == "fused" else 400)
    if kind == "noise":
        bt.set_exact(2)
    before = bt.exact_stats()
    assert before[0]
    got = bt.detect_chains_indexed(d_frames, table, d_starts)
    bt.sync()
    refined = bt.exact_stats()[2] - before[2]
    print(family, kind, "windows refined:", refined, "of", 2 * ns)
    assert refined > 0, "these frames must be re-decided"
    if kind == "noise":
        assert refined == 2 * ns
    plain = bt.detect_chains(d_frames[torch.from_numpy(table).long().cuda()], d_starts)
    bt.sync()
    assert bt.exact_stats()[2] - before[2] == 2 * refined       # the same windows were flagged over the copy
    assert torch.equal(got, plain)
    bt.close()
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    for c in range(2):
        want, g = [], starts[c]
        for f in table[c]:
            g = tuple(oracle.detect(frames[f], 128, K, (ws[0] // 2, ws[1] // 2), g))
            want.append(g)
        assert _as_lists(got)[c] == want, (family, kind, c)
        if kind == "ties":
            assert want == [(centre[f][0], centre[f][1] - sep) for f in table[c]]    # the left speck: the first maximum


# ---- 3. untouched rows, and a start that is kept as given ----
def test_first_one_keeps_an_unclamped_start_and_ended_rows_stay_untouched(pt, oracle):
    import torch
    st = _stack("small")
    table = np.array([[0, 1, 2, -1, -1, -1], [4, -1, -1, -1, -1, -1], [-1] * 6, [6, 7, 8, 9, 10, 11]], np.int32)
    starts = [(-1, 5), (0, st.w + 2), (-500, 9000), (st.h + 3, 40)]      # outside the frame, inside the pad; clip 2's is never used
    d_starts = torch.tensor(starts, dtype=torch.int32).cuda()
    for pin in (lambda bt: None, lambda bt: bt.set_variant(129), lambda bt: bt.set_variant(20)):
        bt = pt.BatchTracker(st.h, st.w, st.tw, (21, 21), True, st.fill(oracle))
        pin(bt)
        out = torch.full((4, 6, 2), SENT, dtype=torch.int32).cuda()
        bt.detect_chains_indexed(st.dev(), table, d_starts, first=1, out=out)
        bt.sync()                                                        # clip 2's start raises nothing: no step uses it
        got = _as_lists(out)
        for c in range(4):
            n = vr.row_len(table[c])
            assert got[c][:n] == st.chain(oracle, table[c], (21, 21), starts[c], 1), c
            assert all(p == (SENT, SENT) for p in got[c][n:]), c
        assert got[0][0] == (-1, 5) and got[1] == [(0, st.w + 2)] + [(SENT, SENT)] * 5 and got[3][0] == (st.h + 3, 40)
        bt.close()


# ---- 4. errors launch nothing ----
def test_indexed_argument_errors_launch_nothing(pt, oracle):
    import torch
    L, E = pt.lib(), pt._lib.PDOG_E_ARG
    st = _stack("small")
    frames = st.dev()
    nf, fs, rs = st.nf, st.h * st.w, st.w
    starts = torch.tensor([[30, 40], [50, 60]], dtype=torch.int32).cuda()
    out = torch.full((2, 6, 2), SENT, dtype=torch.int32).cuda()
    fp, sp, op = (C.c_void_p(t.data_ptr()) for t in (frames, starts, out))
    keep = []

    def tab(v):
        keep.append(np.ascontiguousarray(v, np.int32))
        return C.c_void_p(keep[-1].ctypes.data)

    ok = [[0, 1, 2, 3, 4, 5], [6, 7, 8, -1, -1, -1]]
    for pin in (lambda bt: None, lambda bt: bt.set_variant(129), lambda bt: bt.set_variant(20)):
        bt = pt.BatchTracker(st.h, st.w, st.tw, (21, 21), True, st.fill(oracle))
        pin(bt)
        bt.use_torch_stream()
        h = bt._h
        bad = [(h, fp, fs, rs, nf, tab([[0, 1, 2, 3, 4, nf], ok[1]]), 6, 2, 0, sp, op),             # an entry >= n_frames
               (h, fp, fs, rs, nf, tab([ok[0], [6, 7, 2 ** 31 - 1, -1, -1, -1]]), 6, 2, 0, sp, op),
               (h, fp, fs, rs, nf, tab([ok[0], [6, -1, 8, -1, -1, -1]]), 6, 2, 0, sp, op),          # a non-negative entry behind a negative one
               (h, fp, fs, rs, nf, tab([[-1, 0, 1, 2, 3, 4], ok[1]]), 6, 2, 1, sp, op),
               (h, fp, fs, rs, nf, tab(ok), 6, 2, 2, sp, op), (h, fp, fs, rs, nf, tab(ok), 6, 2, -1, sp, op),   # first
               (None, fp, fs, rs, nf, tab(ok), 6, 2, 0, sp, op), (h, None, fs, rs, nf, tab(ok), 6, 2, 0, sp, op),   # null pointers
               (h, fp, fs, rs, nf, None, 6, 2, 0, sp, op), (h, fp, fs, rs, nf, tab(ok), 6, 2, 0, None, op),
               (h, fp, fs, rs, nf, tab(ok), 6, 2, 0, sp, None),
               (h, fp, fs, rs, 0, tab(ok), 6, 2, 0, sp, op), (h, fp, fs, rs, nf, tab(ok), 0, 2, 0, sp, op),      # sizes and strides
               (h, fp, fs, rs, nf, tab(ok), 6, 0, 0, sp, op), (h, fp, fs, st.w - 1, nf, tab(ok), 6, 2, 0, sp, op),
               (h, fp, -1, rs, nf, tab(ok), 6, 2, 0, sp, op), (h, fp, fs, rs, nf, tab(ok), 2 ** 30, 4, 0, sp, op)]  # n_clips * n_steps beyond int32
        for a in bad:
            assert L.pdog_detect_chains_indexed(*a) == E, a[5:9]
            assert L.pdog_last_error().startswith(b"pdog_detect_chains_indexed")
        bt.sync()                                                        # clean: nothing ran, nothing was raised
        assert (out == SENT).all() and keep
        with pytest.raises(pt.PdogError) as e:                           # the binding hands the library's verdict on
            bt.detect_chains_indexed(frames, [[0, 1, nf]], starts[:1], out=out[:1, :3].contiguous())
        assert e.value.code == E
        for exc, args in ((TypeError, (frames.cpu(), ok, starts)), (TypeError, (frames, [[0.5, 1.0]], starts[:1])),
                          (ValueError, (frames, [0, 1, 2], starts[:1])), (ValueError, (frames, ok, starts[:1])),
                          (TypeError, (frames, ok, starts.long()))):
            with pytest.raises(exc):
                bt.detect_chains_indexed(*args)
        # a guess further outside the frame than the pad: PDOG_E_RANGE from sync(), once, and the tracker stays usable
        hw = bt.info().kernel_len // 2
        far = starts.clone()
        far[1] = torch.tensor([st.h + hw + 2, 10], dtype=torch.int32)
        bt.detect_chains_indexed(frames, ok, far)
        with pytest.raises(pt.PdogError) as e:
            bt.sync()
        assert e.value.code == pt._lib.PDOG_E_RANGE
        bt.sync()
        got = _as_lists(bt.detect_chains_indexed(frames, ok, starts))
        bt.sync()
        assert got[0] == st.chain(oracle, ok[0], (21, 21), (30, 40), 0) and got[1][:3] == st.chain(oracle, ok[1], (21, 21), (50, 60), 0)
        bt.close()


# ---- 5. a fill per clip over a table ----
@pytest.mark.parametrize("first", (0, 1))
def test_track_clips_indexed_three_fills_ragged(pt, oracle, first):
    """Clips of three fills sharing one stack, ragged rows: per step and fill group a batch whose frame index comes from the
    table.  Discs walk near the borders, so the fill decides positions.  Clips of one fill take the chain over the table."""
    import torch
    st = _stack("small")
    ws = (21, 21)
    a = np.arange(6)
    table = np.array([a, a + 2, list(a[:4] + 6) + [-1, -1], [-1] * 6, a[::-1] + 3, [7] + [-1] * 5, a + 6, list(a[:2]) + [-1] * 4], np.int32)
    fills = [30, 128, 220, 30, 128, 220, 30, 128]
    starts = [(3, 5), (st.h - 2, st.w - 4), (2, st.w - 3)] + st.starts(table)[3:]     # three windows hang over the padded frame
    refs = [st.chain(oracle, r, ws, s, first, fill=f) for r, s, f in zip(table, starts, fills)]
    shared = [st.chain(oracle, r, ws, s, first, fill=128) for r, s in zip(table, starts)]
    assert any(x != y for x, y in zip(refs, shared)), "the recipe must make the fill matter"
    d_starts = torch.tensor(starts, dtype=torch.int32).cuda()
    bt = pt.BatchTracker(st.h, st.w, st.tw, ws, True, 7)
    out = torch.full((8, 6, 2), SENT, dtype=torch.int32).cuda()
    got = bt.track_clips_indexed(st.dev(), table, d_starts, fills=fills, first=first, out=out)
    bt.sync()
    assert got is out and bt.info().fill == 7
    lens = [vr.row_len(r) for r in table]
    assert bt.clips_counters()[2:] == (sum(len({f for f, n in zip(fills, lens) if n > k}) for k in range(first, 6)), 0)
    got = _as_lists(out)
    for c, n in enumerate(lens):
        assert got[c][:n] == refs[c], (first, c)
        assert all(p == (SENT, SENT) for p in got[c][n:]), (first, c)
    # one fill: the chain over the table under that fill, counted as the fast path; the tracker's own fill for fills = None
    before = bt.clips_counters()
    one = _as_lists(bt.track_clips_indexed(st.dev(), table, d_starts, fills=[128] * 8, first=first))
    bt.sync()
    assert bt.clips_counters()[2:] == (before[2], before[3] + 1) and bt.info().fill == 7
    bt.set_fill(128)
    own = bt.track_clips_indexed(st.dev(), table, d_starts, first=first)
    assert torch.equal(own, bt.detect_chains_indexed(st.dev(), table, d_starts, first=first))
    bt.sync()
    assert bt.clips_counters()[3] == before[3] + 2
    for c, n in enumerate(lens):
        assert one[c][:n] == shared[c] == _as_lists(own)[c][:n], (first, c)
        assert all(p == (0, 0) for p in one[c][n:]), (first, c)               # a fresh `out` is zeroed
    # errors launch nothing: a bad fill, a bad table
    for bad_fills, bad_table in (([30, 256] + fills[2:], table), (fills, np.where(table == 11, 12, table))):
        with pytest.raises(pt.PdogError) as e:
            bt.track_clips_indexed(st.dev(), bad_table, d_starts, fills=bad_fills, first=first, out=out)
        assert e.value.code == pt._lib.PDOG_E_ARG and "pdog_clips_track_indexed" in str(e.value)
    bt.sync()
    assert _as_lists(out) == got and bt.info().fill == 128
    bt.close()


# ---- 6. track_video ----
def test_track_video_is_track_frames_on_the_selected_frames(pt):
    """A 60-frame clip at 30 frames per second, two discs, 24 positions per second from 0.2 s to 1.7 s: per target the host
    mirror track_frames on the frames the table selects, the restatement's time stamps, Tracker.measure per frame."""
    import torch
    h, w, tw, nf, rate = 120, 160, 25, 60, 30
    rng = np.random.default_rng(23)
    frames = (128 + rng.integers(-2, 3, (nf, h, w))).astype(np.uint8)
    yy, xx = np.ogrid[0:h, 0:w]
    paths = [lambda k: (30 + k, 40 + (3 * k) // 2), lambda k: (100 - k // 4, 30 + k // 2)]      # (never closer than 60 pixels)
    for k in range(nf):
        for p in paths:
            ci, cj = p(k)
            frames[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= 12 * 12] = 5
    start, stop, fps = 0.2, 1.7, 24
    table = vr.fps_table(rate, nf, start, stop, fps)
    assert len(table) == 36 and table[0] == 6 and len(set(table)) == 36
    p0, p1 = paths[0](6), paths[1](6)
    locs = [("ij", (p0[0] + 3, p0[1] - 2)), (float(p1[1] + 2), float(p1[0] - 3)), None]     # a CartesianIndex, an (x, y), missing
    ts, idx, sub = pt.track_video(_cuda(frames), rate, start, stop, fps, tw, locs, subpixel=True)
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.shape == (3, 36, 2) and sub.dtype == torch.float64 and sub.shape == (3, 36, 2)
    assert np.array_equal(ts, vr.time_axis_float(start, stop, fps)[:36]) and ts.dtype == np.float64
    got, gsub = _as_lists(idx), sub.cpu().numpy()
    selected = [frames[i] for i in table]
    for k, loc in enumerate(locs):
        want, wsub = pt.track_frames(selected, tw, loc, subpixel=True)
        assert got[k] == [tuple(p) for p in want], k
        assert [tuple(r) for r in gsub[k]] == [tuple(r) for r in wsub], k
    assert got[0] != got[1] and max(abs(a - b) for p, q in zip(got[0], [paths[0](i) for i in table]) for a, b in zip(p, q)) <= 3
    ts2, idx2 = pt.track_video(_cuda(frames), rate, start, stop, fps, tw, locs[1])          # one location, no sub-pixel positions
    assert np.array_equal(ts2, ts) and torch.equal(idx2[0], idx[1]) and idx2.shape == (1, 36, 2)
    ts3, idx3 = pt.track_video(_cuda(frames), rate, 1.0, pt.DEFAULT_STOP, fps, tw)          # the stack ends before stop
    t3 = vr.fps_table(rate, nf, 1.0, BIG, fps)
    assert len(ts3) == len(t3) == idx3.shape[1] and np.array_equal(ts3, vr.time_axis_float(1.0, BIG, fps)[:len(t3)])
    assert _as_lists(idx3)[0] == [tuple(p) for p in pt.track_frames([frames[i] for i in t3], tw, None)]


# ---- 7. the host orchestration's rarely taken branches ----
def test_progress_chain_on_kernels_that_arm_no_ticket(pt, oracle):
    """The batch kernels (the l = 29 ring and roll instances pinned) publish no ticket of their own: the stepped walk queues
    a publishing kernel behind every step.  The positions equal detect_chain's on the same pinned tracker and the oracle's
    chain, and the counter ends at the number of frames."""
    st, ws, nf = _stack("small"), (21, 21), 8
    frames, row = st.dev()[:nf], list(range(nf))
    start = st.starts([row])[0]
    want = st.chain(oracle, row, ws, start, 0)
    bt = pt.BatchTracker(st.h, st.w, st.tw, ws, True, st.fill(oracle))
    try:
        for variant in (20, 129):
            bt.set_variant(variant)
            assert bt.info().variant == variant and bt.kernel_for_batch(1) == variant
            plain = bt.detect_chain(frames, start)
            bt.sync()
            cp = bt.detect_chain_progress(frames, start)
            got = cp.wait()
            assert cp.done() == nf, variant
            assert [tuple(int(v) for v in p) for p in got] == want == _as_lists(plain[None])[0], variant
            cp.close()
    finally:
        bt.close()


def test_back_to_back_table_uploads_need_no_sync_between(pt, oracle):
    """Two (then three) indexed calls on the per-step batches (variant 20 is the l = 29 ring kernel: the table goes up
    step-major, dog_chain_table_init_kernel, then a batch and a step kernel per step) with nothing waiting between them:
    the second table is larger and grows the staging, the third is packed into staging that the second's upload may still
    be reading.  After one sync every output equals what its call gives alone, and the restatement."""
    import torch
    st, ws = _stack("small"), (21, 21)
    tabs = _tables(st.nf, 6)
    tables = [np.asarray(tabs[name], np.int32) for name in ("identity", "ragged", "identity")]
    starts = [st.starts(tb) for tb in tables]
    d_starts = [torch.tensor(s, dtype=torch.int32).cuda() for s in starts]
    outs = [torch.full(tb.shape + (2,), SENT, dtype=torch.int32).cuda() for tb in tables]
    alone = [torch.full(tb.shape + (2,), SENT, dtype=torch.int32).cuda() for tb in tables]
    frames = st.dev()
    bt = pt.BatchTracker(st.h, st.w, st.tw, ws, True, st.fill(oracle))
    try:
        bt.set_variant(20)
        assert bt.info().variant == 20
        bt.sync()
        for tb, s, o in zip(tables, d_starts, outs):
            bt.detect_chains_indexed(frames, tb, s, out=o)
        bt.sync()
        for tb, s, o in zip(tables, d_starts, alone):
            bt.detect_chains_indexed(frames, tb, s, out=o)
            bt.sync()
    finally:
        bt.close()
    for tb, s, o, a in zip(tables, starts, outs, alone):
        got = _as_lists(o)
        assert got == _as_lists(a)
        for c, row in enumerate(tb):
            n = vr.row_len(row)
            assert got[c][:n] == st.chain(oracle, row, ws, s[c], 0), c
            assert all(p == (SENT, SENT) for p in got[c][n:]), c


def test_back_to_back_clip_plans_need_no_sync_between(pt, oracle):
    """The same for the clips handle: two calls of two fills each (so each uploads a plan), the second with more clips,
    nothing waiting between them.  Each equals its own result when run alone, and the restatement under each clip's fill."""
    import torch
    st, ws = _stack("small"), (21, 21)
    a = np.arange(6)
    calls = [(np.array([a, a + 2], np.int32), [30, 128]),
             (np.array([a + 6, a[::-1] + 3, list(a[:4]) + [-1, -1], a + 1, [7] + [-1] * 5], np.int32), [128, 30, 128, 30, 30])]
    starts = [st.starts(tb) for tb, _ in calls]
    d_starts = [torch.tensor(s, dtype=torch.int32).cuda() for s in starts]
    outs = [torch.full(tb.shape + (2,), SENT, dtype=torch.int32).cuda() for tb, _ in calls]
    alone = [torch.full(tb.shape + (2,), SENT, dtype=torch.int32).cuda() for tb, _ in calls]
    frames = st.dev()
    bt = pt.BatchTracker(st.h, st.w, st.tw, ws, True, 7)
    try:
        bt.clip_modes(frames[:1])          # the handle exists before the calls under test
        bt.sync()
        before = bt.clips_counters()
        for (tb, fills), s, o in zip(calls, d_starts, outs):
            bt.track_clips_indexed(frames, tb, s, fills=fills, out=o)
        bt.sync()
        assert bt.clips_counters()[3] == before[3]       # neither call took the one-fill fast path
        for (tb, fills), s, o in zip(calls, d_starts, alone):
            bt.track_clips_indexed(frames, tb, s, fills=fills, out=o)
            bt.sync()
    finally:
        bt.close()
    for (tb, fills), s, o, al in zip(calls, starts, outs, alone):
        got = _as_lists(o)
        assert got == _as_lists(al)
        for c, row in enumerate(tb):
            n = vr.row_len(row)
            assert got[c][:n] == st.chain(oracle, row, ws, s[c], 0, fill=fills[c]), c
            assert all(p == (SENT, SENT) for p in got[c][n:]), c
