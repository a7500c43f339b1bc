"""Exact mode's positions on hard windows, per kernel family and kernel length: the census.

Exact mode (csrc/dog_exact.hpp) promises the dense Float64 oracle's position for every window.  Three links must hold per
family and length: the threshold T exact_factors derives from the family's operation order, the flag with its candidate set
(runner-up tracking, column masks, strip slots, the folded column, the response-map and the rescan routes), and the Float64
re-evaluation (exact_pixel / exact_patch, the inline refinements of the fused, tiled and chain kernels, the finishing
kernel).  tests/test_gpu_exact.py holds that chain at l = 65 on 45 x 45 windows; here it is held for
    roll        l = 17 ... 149 (both sides of the three-waves / two-waves boundary at 101): a partial strip (21 x 45), two strips
                plus three thin columns (21 x 131) through the map and the rescan route, local dc, bright targets, `no_prune`,
                the folded column (21 x 65 under `fold_always` / `no_fold`, 21 x 513 folded unasked), the persistent chains
    ring        variants 0, 1, 2, 10, 13 (l = 65) and 20 (l = 29)
    fused       l = 29 ... 101, compile-time and runtime-length instances, both signs, local dc, detect_chain
    tiled       l = 29, 65, 101 as the tracker's own choice for one and two 96 x 81 windows, detect_chain
    two-pass    plain (l = 29, 65) and blocked (l = 101, 113, 125, 293): two windows, twenty, `twopass_4l`, map and rescan route
    the host functor at l = 29 and 101
on tests/exact_scenes.py's windows: noise only, a one-level target, two near-equal blobs, exact ties, tiles over borders and
corners, and an easy control.  tests/test_exact_scenes_cpu.py shows on the CPU that a kernel which only ranks its FP32 responses
answers wrongly on a share of every set, and that the windows of families 0, 1 and 3 lie under the flag rule.

Every case pins its kernel (set_variant, kernel_for_batch), runs with set_exact(1), compares EVERY window's position with the
dense oracle's (equality), asserts that windows were refined, runs again with set_exact(0) only to print how many raw positions
differ, and prints one `census` line (profiles/exact_lengths_census.txt).  PARITY UNPINNED: the oracle is this repository's
restatement (oracle/dog_oracle.c)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_scenes as xs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_USED = []


def _scene(oracle, S):
    """The Set's scene and the dense oracle's positions — of a Set tests/test_exact_scenes_cpu.py has shown to be hard."""
    if not _USED:
        _USED.extend(xs.used_sets(oracle))
    assert S in _USED, xs.label(S)
    return xs.evaluate(oracle, S)


def _pinned(pt, S, ev, variant, tuning, exact):
    fh, fw = ev["frames"].shape[1:]
    bt = pt.BatchTracker(fh, fw, ev["tw"], S.ws, S.darker, xs.CONTENTS[S.content][1])
    try:
        assert bt.info().kernel_len == S.l
        if variant is not None:
            bt.set_variant(variant)
        for key, value in tuning:
            bt.set_tuning(key, value)
        bt.set_exact(exact)
    except Exception:
        bt.close()
        raise
    return bt


def _line(family, S, variant, n, tuning, route, refined, raw):
    note = " ".join(f"{k}={v}" for k, v in tuning) or "-"
    print(f"census {family:8s} l={S.l:3d} {S.ws[0]}x{S.ws[1]} variant={variant} n={n} {S.content} {'dark' if S.darker else 'bright'} "
          f"{note} route={route}: refined {refined}, raw FP32 positions that differ from the dense oracle {raw}")


def _census(pt, oracle, family, S, kernel, variant=None, tuning=(), n=None, groups=None, repeat=1, route="default"):
    """The first n windows of S (all of them by default) in one launch — `groups`: in these launches —, `repeat` times on one
    tracker: every position of every repetition equals the dense oracle's and windows were refined.  Returns (positions, refined)."""
    ev = _scene(oracle, S)
    n = S.n if n is None else n
    guesses, dense = ev["guesses"], ev["dense"][:n]
    groups = [np.arange(n)] if groups is None else [np.asarray(g) for g in groups]
    assert sorted(np.concatenate(groups).tolist()) == list(range(n))
    d_frames = _cuda(ev["frames"])
    result = {}
    for exact in (1, 0):
        bt = _pinned(pt, S, ev, variant, tuning, exact)
        try:
            runs = []
            for _ in range(repeat):
                got = np.zeros((n, 2), np.int32)
                for idx in groups:
                    assert bt.kernel_for_batch(len(idx)) == kernel, (family, xs.label(S), len(idx), bt.kernel_for_batch(len(idx)))
                    out = bt.detect(d_frames, _cuda(guesses[idx]), _cuda(idx.astype(np.int32)))
                    bt.sync()
                    got[idx] = out.cpu().numpy()
                runs.append(got)
            result[exact] = (runs, bt.exact_stats()[2])
        finally:
            bt.close()
    runs, refined = result[1]
    raw = int((result[0][0][0] != dense).any(1).sum())
    _line(family, S, variant, n, tuning, route, refined, raw)
    for r, got in enumerate(runs):
        bad = np.flatnonzero((got != dense).any(1))
        assert bad.size == 0, (family, xs.label(S), variant, tuning, route, "run", r, "windows", bad.tolist(), "families", ev["fam"][bad].tolist(),
                               got[bad][:6].tolist(), dense[bad][:6].tolist())
    assert refined > 0, (family, xs.label(S), variant, tuning)
    return runs[0], refined


def _chain(pt, oracle, family, S, kernel, variant=None, tuning=(), clips=1):
    """detect_chain (one clip) or detect_chains over the Set's frames, cut into `clips` clips that start at their first
    frame's guess: positions equal the dense oracle's chain step by step."""
    ev = _scene(oracle, S)
    nf = S.n // clips
    fh, fw = ev["frames"].shape[1:]
    starts = ev["guesses"][::nf][:clips]
    want = np.stack([xs.oracle_chain(oracle, S, c, nf, starts[c]) for c in range(clips)])
    d_frames = _cuda(ev["frames"][:clips * nf].reshape(clips, nf, fh, fw))
    result = {}
    for exact in (1, 0):
        bt = _pinned(pt, S, ev, variant, tuning, exact)
        try:
            assert bt.kernel_for_batch(clips) == kernel, (family, xs.label(S), bt.kernel_for_batch(clips))
            if clips == 1:
                got = bt.detect_chain(d_frames[0], (int(starts[0][0]), int(starts[0][1]))).cpu().numpy()[None]
            else:
                got = bt.detect_chains(d_frames, _cuda(starts)).cpu().numpy()
            bt.sync()
            result[exact] = (got, bt.exact_stats()[2])
        finally:
            bt.close()
    got, refined = result[1]
    raw = int((result[0][0] != want).any(2).sum())
    _line(family + "-chain", S, variant, f"{clips}x{nf}", tuning, "default", refined, raw)
    assert np.array_equal(got, want), (family, xs.label(S), variant, tuning, np.argwhere((got != want).any(2))[:6].tolist())
    assert refined > 0, (family, xs.label(S), variant, tuning)


def _rescan(monkeypatch):
    """The refinement's candidates recomputed instead of read off a response map: PDOG_MAP_MB=0 (read at create) and, for
    the roll kernels, `no_roll_map`."""
    monkeypatch.setenv("PDOG_MAP_MB", "0")


# ---- roll: dog_roll_kernel, dog_thin_kernel, the folded column ----
@pytest.mark.parametrize("content", ["fill", "local dc"])
@pytest.mark.parametrize("l", xs.ROLL_LENGTHS)
def test_roll_partial_strip(pt, oracle, l, content):
    vid = xs.roll_variant(l)
    _census(pt, oracle, "roll", xs.roll_set(l, xs.P, content), vid, variant=vid)


@pytest.mark.parametrize("l", xs.ROLL_BRIGHT)
def test_roll_bright_targets(pt, oracle, l):
    vid = xs.roll_variant(l)
    _census(pt, oracle, "roll", xs.roll_set(l, xs.P, darker=False), vid, variant=vid)


@pytest.mark.parametrize("route", ["map", "rescan"])
@pytest.mark.parametrize("l", xs.ROLL_LENGTHS)
def test_roll_two_strips_and_thin_columns(pt, oracle, monkeypatch, l, route):
    """21 x 131: two strips plus three thin columns; family 2's pairs lie across the strip boundary and in the thin columns.
    map: the second launch on the tracker reads its candidates off the response map; rescan: they are recomputed."""
    vid = xs.roll_variant(l)
    if route == "rescan":
        _rescan(monkeypatch)
        _census(pt, oracle, "roll", xs.roll_set(l, xs.X), vid, variant=vid, tuning=(("no_roll_map", 1),), repeat=2, route=route)
    else:
        _census(pt, oracle, "roll", xs.roll_set(l, xs.X), vid, variant=vid, repeat=2, route=route)


@pytest.mark.parametrize("l", xs.ROLL_NO_PRUNE)
def test_roll_no_prune_changes_nothing(pt, oracle, l):
    vid = xs.roll_variant(l)
    S = xs.roll_set(l, xs.P)
    pos, refined = _census(pt, oracle, "roll", S, vid, variant=vid)
    pos_d, refined_d = _census(pt, oracle, "roll", S, vid, variant=vid, tuning=(("no_prune", 1),))
    assert np.array_equal(pos, pos_d) and refined == refined_d, (l, refined, refined_d)


@pytest.mark.parametrize("switch", ["fold_always", "no_fold"])
def test_roll_single_remainder_column(pt, oracle, switch):
    """21 x 65 at l = 65: one remainder column — folded into the last strip (fold_column_peak under a flag) or left to the thin
    kernel; a quarter of family 2's pairs have their second disc centred on it."""
    _census(pt, oracle, "roll", xs.roll_set(65, (21, 65)), 100, variant=100, tuning=((switch, 1),))


def test_roll_eight_strips_fold_unasked(pt, oracle):
    S = xs.roll_set(65, (21, 513), n=8)
    ev = _scene(oracle, S)
    bt = _pinned(pt, S, ev, 100, (), 1)
    strips = bt.info().n_strips
    bt.close()
    assert strips == 8                                          # (what dog_roll's automatic fold asks for)
    _census(pt, oracle, "roll", S, 100, variant=100)


@pytest.mark.parametrize("l", xs.CHAIN_LENGTHS)
def test_roll_persistent_chains(pt, oracle, l):
    """8 clips x 6 noise-only frames, 21 x 131 windows: every step is a near-tie."""
    vid = xs.roll_variant(l)
    _chain(pt, oracle, "roll", xs.roll_chain_set(l), vid, variant=vid, clips=8)


# ---- ring: dog_window_kernel and the finishing kernel ----
@pytest.mark.parametrize("variant,l", xs.RING)
def test_ring(pt, oracle, variant, l):
    _census(pt, oracle, "ring", xs.ring_set(l), variant, variant=variant)


# ---- fused: dog_fused_kernel, inline refinement ----
@pytest.mark.parametrize("no_fused_c", [0, 1])
@pytest.mark.parametrize("l", xs.FUSED_LENGTHS)
def test_fused(pt, oracle, l, no_fused_c):
    tuning = (("no_fused_c", no_fused_c),)
    _census(pt, oracle, "fused", xs.fused_set(l), 300, variant=300, tuning=tuning)
    if l in xs.FUSED_BRIGHT:
        _census(pt, oracle, "fused", xs.fused_set(l, darker=False), 300, variant=300, tuning=tuning)
    if l == 65:
        _census(pt, oracle, "fused", xs.fused_set(l, "local dc"), 300, variant=300, tuning=tuning)


@pytest.mark.parametrize("no_fused_c", [0, 1])
@pytest.mark.parametrize("l", xs.FUSED_LENGTHS)
def test_fused_chain(pt, oracle, l, no_fused_c):
    _chain(pt, oracle, "fused", xs.fused_chain_set(l), 300, variant=300, tuning=(("no_fused_c", no_fused_c),))


# ---- tiled: dog_tiled_kernel, the tracker's own choice ----
@pytest.mark.parametrize("l", xs.TILED_LENGTHS)
def test_tiled(pt, oracle, l):
    """96 x 81 windows: six launches of two windows and two of one; family 2's discs lie at least 24 rows and columns apart,
    more than a sub-window's edge."""
    groups = [[2 * k, 2 * k + 1] for k in range(6)] + [[12], [13]]
    _census(pt, oracle, "tiled", xs.tiled_set(l), 400, groups=groups)


@pytest.mark.parametrize("l", xs.TILED_LENGTHS)
def test_tiled_chain(pt, oracle, l):
    _chain(pt, oracle, "tiled", xs.tiled_chain_set(l), 400)


# ---- two-pass: dog_h1_kernel + dog_hpass_kernel, the refinement kernel ----
@pytest.mark.parametrize("route", ["map", "rescan"])
@pytest.mark.parametrize("l,ws", xs.TWOPASS)
def test_twopass(pt, oracle, monkeypatch, l, ws, route):
    """n = 2: the small-batch form; n = 20: the four-launch form; `twopass_4l`: that form for two windows."""
    if route == "rescan":
        _rescan(monkeypatch)
    S = xs.twopass_set(l, ws)
    for n, tuning in ((2, ()), (20, ()), (2, (("twopass_4l", 1),))):
        _census(pt, oracle, "twopass", S, 200, variant=200, tuning=tuning, n=n, repeat=2 if route == "map" else 1, route=route)


# ---- the host functor ----
@pytest.mark.parametrize("l", xs.FUNCTOR_LENGTHS)
def test_host_functor(pt, oracle, l):
    """Tracker(frame, tw, default window, darker)(guess) on noise-only and one-level frames: the ticket goes out after the
    refinement.  The fill is the mode of the frame, as the reference's constructor takes it."""
    tw = xs.tw_for_kernel_len(l)
    window = pt.guess_window_size(tw)
    assert window == oracle.default_window(tw)
    S = xs.functor_set(l, window)
    ev = _scene(oracle, S)
    refined = raw = 0
    got = []
    for b in range(S.n):
        t = pt.Tracker(ev["frames"][b], tw, S.ws, S.darker)
        try:
            assert t.info().kernel_len == l and t.img.fillvalue == ev["fills"][b]
            kernel = t.kernel_for_batch(1)
            g = (int(ev["guesses"][b][0]), int(ev["guesses"][b][1]))
            got.append(t(g))
            refined += t.exact_stats()[2]
            t.set_exact(0)
            raw += t(g) != tuple(ev["dense"][b])
        finally:
            t.close()
    _line("functor", S, kernel, 1, (), "default", refined, raw)
    assert kernel == 300 or l != 29      # (21 x 21 at l = 29 is the fused kernel's; the census line names what served 69 x 69 at l = 101)
    assert got == [tuple(p) for p in ev["dense"].tolist()], (l, got, ev["dense"].tolist())
    assert refined > 0
