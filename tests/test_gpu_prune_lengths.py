"""Every compiled PRUNE instance of the roll kernel (csrc/dog_roll.hpp, one per kernel length l = 17, 21, … 149) and the pre-pass
(csrc/dog_prune.hpp) under every form of kept range, for dark and bright targets, with exact mode on and off, and pruned and
dense launches interleaved on one tracker.  Everything is decided by exact equality.

The scenes are tests/prune_length_scenes.py's: ten windows of (2 l + 29) × 131 per length, in which the restatement
(tests/prune_restatement.py) finds every class of kept range — a range that starts at sub-chunk 0, inside the shortened
prologue bodies, at a full body (three phases of the ring at least), that ends at the window's last block, an empty strip
beside a kept one, remainder columns kept from a later block and empty.  tests/test_prune_lengths_cpu.py shows that on the CPU.

Per length (test_kept_ranges_at_every_length; bright targets: test_bright_targets_kept_ranges):
  * the ten windows as one batch, pruning on and `no_prune`, exact mode on: positions equal each other and the dense Float64
    oracle's, the merged FP32 maxima are bit-equal, exact mode re-evaluated as many windows, `no_prune` counted nothing and the
    pruned run counted exactly the restatement's (kept, total) (slot, sub-chunk) pairs.  The `no_prune` run is the plain
    instance in batch form, without the response map;
  * each window as a batch of its own on a fresh tracker: the restatement's counts of that window and the oracle's position —
    a failure names the window, and prune_length_scenes._placements says which class it was built for;
  * exact mode off: pruned and `no_prune` agree in positions and maxima, the counts are the restatement's.
Measured on an MI355X: 0.03 s (l = 21) to 0.46 s (l = 149) per length, nearly all of it the oracle and the restatement
(the fifteen trackers and their launches take 0.02 … 0.03 s); the file's 40 tests together 9 s.

What no result can show: whether roll_strip holds the outputs above row 8·ba back from the peak.  Such an output is the exact
response of the tile with the rows above sub-chunk ba set to the DC level; its block's energy only shrinks by that, so the
pre-pass's own bound keeps it below the maximum − T_max.  A scratch build with y_lo = 0 passes every test here and before.
A scratch build with prune_tail one too small fails every scene set, 18 of the 38 by a moved position, the rest by the
counts; one with the sign of the 3 × 3-cell sums dropped moves the counts of every dark set, one with the sign always applied
those of the bright sets only (which no earlier test notices).

test_bright_complement_of_the_disc_batch: the complement of tests/test_gpu_prune.py's 64-window disc batch at l = 65, bright targets.

test_pruned_and_dense_launches_interleaved: l = 65, windows of 41 × 513 (eight strips and one remainder column: the dense
launch folds the column into the last strip, the pruned one keeps the thin kernel), one tracker.  A disc batch D, a
noise-only batch Q, then D again: Q's counts put PrunePolicy (csrc/pdog_policy.hpp) to sleep, the next kPruneProbeEvery
eligible batches run dense, the one after probes.  The schedule is derived from a restatement of PrunePolicy::decide fed
with the counts the restatement of the pre-pass gives, and held through prune_counts(); every call returns the oracle's
positions and the maxima of the first pruned call, whichever form served it, at batch sizes 8, 3, 8, … among the dense calls
(LaunchGeo::part_mask holds kept ranges in one launch and column masks in the next, d_fold_r is reused at another size)."""
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
from test_gpu_prune import _disc_batch, _tw_for_kernel_len  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


class _Tracker:
    """One pinned roll tracker; run() is one batch call followed by sync()."""

    def __init__(self, pt, fh, fw, l, ws, darker, fill, exact=1, **tuning):
        self.bt = pt.BatchTracker(fh, fw, _tw_for_kernel_len(l), ws, darker, fill)
        self.vid = ps.variant_id(l)
        assert self.bt.info().kernel_len == l
        self.bt.set_variant(self.vid)
        for key, value in tuning.items():
            self.bt.set_tuning(key, value)
        self.bt.set_exact(exact)

    def run(self, frames, guesses):
        """(positions, maxima, windows exact mode re-evaluated so far, prune_counts so far)."""
        import torch
        n = len(frames)
        assert self.bt.kernel_for_batch(n) == self.vid
        pos = self.bt.detect(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), torch.from_numpy(np.ascontiguousarray(guesses)).cuda())
        self.bt.sync()
        return pos.cpu().numpy(), self.bt.batch_maxima(n), self.bt.exact_stats()[2], self.bt.prune_counts()

    def close(self):
        self.bt.close()


def _once(pt, fh, fw, l, ws, darker, fill, frames, guesses, exact, **tuning):
    t = _Tracker(pt, fh, fw, l, ws, darker, fill, exact, **tuning)
    try:
        return t.run(frames, guesses)
    finally:
        t.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_CACHE = {}


def _case(oracle, l, darker):
    """Scenes, the oracle's positions and the restatement's pre-pass of one length and sign: built once."""
    if (l, darker) not in _CACHE:
        frames, guesses, fill = ps.scenes(l, darker)
        tw = _tw_for_kernel_len(l)
        sg = oracle.sigma(tw)
        assert oracle.kernel_len(sg) == l
        ref = oracle.detect_batch_par(frames, fill, oracle.dog_kernel(sg, darker), sg, darker, ps.geometry(l)[2], guesses, separable=False)
        _CACHE[(l, darker)] = (frames, guesses, fill, ref, ps.restate(l, darker, frames, guesses, fill))
    return _CACHE[(l, darker)]


def _kept_ranges(pt, oracle, l, darker):
    t0 = time.perf_counter()
    frames, guesses, fill, ref, pps = _case(oracle, l, darker)
    t1 = time.perf_counter()
    fh, ws = ps.geometry(l)[0], ps.geometry(l)[1]
    per_window = ps.counts(l, pps)
    want = (sum(k for k, _ in per_window), sum(t for _, t in per_window))
    found = ps.classes_of(l, pps)
    assert all(found[c] for c in ps.CLASSES), l                               # (tests/test_prune_lengths_cpu.py shows it for every length)
    assert all(0 < k < t for k, t in per_window), (l, per_window)
    args = (pt, fh, ps.FW, l, ws, darker, fill)
    # the whole set: pruned against `no_prune`, exact mode on
    pos_p, max_p, ref_p, counts_p = _once(*args, frames, guesses, 1, no_prune=0)
    pos_d, max_d, ref_d, counts_d = _once(*args, frames, guesses, 1, no_prune=1)
    sign = "dark" if darker else "bright"
    print(f"prune lengths l={l} {sign}: kept {counts_p[0]} of {counts_p[1]} (slot, sub-chunk) pairs, the restatement {want[0]} of {want[1]}; "
          f"windows refined {ref_p} / {ref_d}")
    assert np.array_equal(pos_d, ref), (l, np.argwhere(pos_d != ref)[:4])     # the plain instance in batch form, no map
    assert np.array_equal(pos_p, pos_d), (l, np.argwhere(pos_p != pos_d)[:4])
    assert np.array_equal(pos_p, ref), (l, np.argwhere(pos_p != ref)[:4])
    assert np.array_equal(_bits(max_p), _bits(max_d)), (l, np.argwhere(max_p != max_d)[:4])
    assert ref_p == ref_d
    assert counts_d == (0, 0)
    assert counts_p == want, (l, counts_p, want)
    # each window alone, a fresh tracker each: a failure names the window
    for w in range(len(frames)):
        pos, mx, _, counts = _once(*args, frames[w:w + 1], guesses[w:w + 1], 1, no_prune=0)
        assert counts == per_window[w], (l, w, counts, per_window[w], pps[w]["hull"])
        assert np.array_equal(pos, ref[w:w + 1]), (l, w, pos, ref[w], pps[w]["hull"])
        assert _bits(mx)[0] == _bits(max_d)[w], (l, w, pps[w]["hull"])
    # exact mode off: the FP32 argmax must not move
    pos_p0, max_p0, _, counts_p0 = _once(*args, frames, guesses, 0, no_prune=0)
    pos_d0, max_d0, _, counts_d0 = _once(*args, frames, guesses, 0, no_prune=1)
    assert np.array_equal(pos_p0, pos_d0), (l, np.argwhere(pos_p0 != pos_d0)[:4])
    assert np.array_equal(_bits(max_p0), _bits(max_d0)) and np.array_equal(_bits(max_p0), _bits(max_p))
    assert counts_d0 == (0, 0) and counts_p0 == want, (l, counts_p0, want)
    t2 = time.perf_counter()
    print(f"prune lengths l={l} {sign}: scenes, oracle and restatement {t1 - t0:.2f} s, GPU runs {t2 - t1:.2f} s")
    return per_window


@pytest.mark.parametrize("l", ps.LENGTHS)
def test_kept_ranges_at_every_length(pt, oracle, l):
    _kept_ranges(pt, oracle, l, True)


@pytest.mark.parametrize("l", (17, 65, 109, 149))
def test_bright_targets_kept_ranges(pt, oracle, l):
    per_window = _kept_ranges(pt, oracle, l, False)
    # the window with a disc of either sign: the kernel kept what the right sign of the cell sums keeps (asserted per window
    # above), which is not what the wrong sign would keep
    frames, guesses, fill, _, pps = _case(oracle, l, False)
    tile = ps.tiles(l, frames, guesses, fill)[ps.TWO_SIGN]
    wrong = pr.kept_pairs(pr.prepass(tile, fill, _tw_for_kernel_len(l), False, cell_darker=True), l)
    assert per_window[ps.TWO_SIGN] == pr.kept_pairs(pps[ps.TWO_SIGN], l) and per_window[ps.TWO_SIGN] != wrong


def test_bright_complement_of_the_disc_batch(pt, oracle):
    l, n, fill, darker = 65, 129, 127, False
    dark, guesses = _disc_batch(l, n)
    frames = (255 - dark).astype(np.uint8)
    fh, fw = frames.shape[1:]
    tw, r = _tw_for_kernel_len(l), n // 2
    ref = oracle.detect_batch(frames, fill, oracle.dog_kernel(oracle.sigma(tw), darker), (r, r), guesses)
    kept = total = 0
    for f, g in zip(frames, guesses):
        k, t = pr.kept_pairs(pr.prepass(fr.window_tile(f, fill, l, (r, r), g), fill, tw, darker), l)
        kept, total = kept + k, total + t
    assert kept < total
    args = (pt, fh, fw, l, (n, n), darker, fill)
    pos_p, max_p, ref_p, counts_p = _once(*args, frames, guesses, 1, no_prune=0)
    pos_d, max_d, ref_d, counts_d = _once(*args, frames, guesses, 1, no_prune=1)
    print(f"prune bright complement l={l} window={n}: kept {counts_p[0]} of {counts_p[1]}, the restatement {kept} of {total}")
    assert np.array_equal(pos_p, ref) and np.array_equal(pos_d, ref), np.argwhere(pos_p != ref)[:4]
    assert np.array_equal(_bits(max_p), _bits(max_d)) and ref_p == ref_d
    assert counts_d == (0, 0) and counts_p == (kept, total)


# ---- pruned and dense launches interleaved ----
class _PrunePolicy:
    """csrc/pdog_policy.hpp, PrunePolicy::decide, on the cumulative counts as Python integers (tests/policy_main.cpp's model)."""

    def __init__(self):
        hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pawsometracker.jl_amd", "csrc", "pdog_policy.hpp")).read()
        self.pre_pct = int(re.search(r"constexpr int kPrunePrePct = (\d+);", hdr).group(1))
        self.probe_every = int(re.search(r"constexpr int kPruneProbeEvery = (\d+);", hdr).group(1))
        self.kept_last = self.total_last = self.sleep = 0

    def decide(self, kept, total):
        dk, dt = kept - self.kept_last, total - self.total_last
        if dt > 0:
            self.kept_last, self.total_last = kept, total
            self.sleep = self.probe_every if dk * 100 > dt * (100 - self.pre_pct) else 0
        if self.sleep > 0:
            self.sleep -= 1
            return False
        return True


def test_pruned_and_dense_launches_interleaved(pt, oracle):
    l, ws, fh, fw, fill, nwin = 65, (41, 513), 120, 700, 128, 8
    tw, radii = _tw_for_kernel_len(l), (ws[0] // 2, ws[1] // 2)
    rad = max(2, int(tw) // 2)
    rng = np.random.default_rng(65513)
    ii, jj = np.ogrid[:fh, :fw]

    def noise(f, a):
        return np.clip(f.astype(np.int16) + rng.integers(-a, a + 1, f.shape), 0, 255).astype(np.uint8)
    guesses = np.array([(60 + (k % 3) - 1, 350 + 2 * k - 7) for k in range(nwin)], np.int32)
    # D: a disc per window, from the first strip to the folded column (window column 512) and across strip boundaries
    cols = (-240, -192, -100, -3, 64, 130, 250, 256)
    D = np.stack([noise(np.where((ii - (g[0] - 1 + 3 * (k % 4) - 5)) ** 2 + (jj - (g[1] - 1 + c)) ** 2 <= rad * rad, 0, fill).astype(np.uint8), 2)
                  for k, (g, c) in enumerate(zip(guesses, cols))])
    Q = np.stack([noise(np.full((fh, fw), fill, np.uint8), 3) for _ in range(nwin)])
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    ref = {"D": oracle.detect_batch(D, fill, K, radii, guesses), "Q": oracle.detect_batch(Q, fill, K, radii, guesses)}
    data = {"D": D, "Q": Q}

    def restated(frames):
        pairs = [pr.kept_pairs(pr.prepass(fr.window_tile(f, fill, l, radii, g), fill, tw, True), l) for f, g in zip(frames, guesses)]
        return sum(k for k, _ in pairs), sum(t for _, t in pairs)
    cnt = {"D": restated(D), "Q": restated(Q)}
    policy = _PrunePolicy()
    assert cnt["D"][0] * 100 < cnt["D"][1] * (100 - policy.pre_pct) and cnt["Q"][0] == cnt["Q"][1], cnt   # a property of the inputs
    assert pr.slots(ws[1]) == [(64 * s, 64) for s in range(8)] + [(512, 1)]                               # eight strips, one remainder column

    # the calls: D, Q, D, then dense calls at sizes 8, 3, 8, … of D and now and then Q until the policy probes, and two calls more
    calls = [("D", 0, 8), ("Q", 0, 8), ("D", 0, 8)]
    k = 0
    while len(calls) < 2 + policy.probe_every + 2:
        calls.append([("D", 0, 8), ("D", 0, 3), ("D", 0, 8), ("D", 5, 8), ("Q", 0, 8), ("D", 2, 5)][k % 6])
        k += 1
    calls[-3:] = [("D", 0, 3), ("D", 0, 8), ("D", 0, 8)]    # the last dense call a small one, then the probe and the batch after it
    # (every noise-only window of Q is a near-tie that exact mode re-evaluates; MapPolicy would answer with the response map, whose
    # launches cannot prune and are no observation for PrunePolicy.  `no_roll_map` keeps the schedule PrunePolicy's alone; the
    # map's launches are tests/test_gpu_exact.py's subject)
    main = _Tracker(pt, fh, fw, l, ws, True, fill, 1, no_roll_map=1)
    unfolded = _Tracker(pt, fh, fw, l, ws, True, fill, 1, no_prune=1, no_fold=1)   # dense, the column on the thin kernel
    t0 = time.perf_counter()
    try:
        kept = total = 0
        first = {}
        forms = []
        for i, (name, a, b) in enumerate(calls):
            pruned = policy.decide(kept, total)                  # (sync() after every call: the counts are published before the next)
            forms.append(pruned)
            if pruned:
                assert (a, b) == (0, 8)                          # (the partial batches are all dense ones: cnt holds whole batches)
                kept, total = kept + cnt[name][0], total + cnt[name][1]
            pos, mx, refined, counts = main.run(data[name][a:b], guesses[a:b])
            if pruned or i < 3:
                print(f"prune interleaved call {i}: {name}[{a}:{b}] {'pruned' if pruned else 'dense'}; counts {counts}; windows refined so far {refined}")
            assert counts == (kept, total), (i, name, (a, b), pruned, counts, (kept, total))
            assert np.array_equal(pos, ref[name][a:b]), (i, name, (a, b), pruned)
            if name not in first:
                assert pruned
                first[name] = mx.copy()
            assert np.array_equal(_bits(mx), _bits(first[name][a:b])), (i, name, (a, b), pruned)
            if i in (2, 3, 4, 7):                                # the same dense calls without the fold
                pos_u, mx_u, _, counts_u = unfolded.run(data[name][a:b], guesses[a:b])
                assert counts_u == (0, 0) and np.array_equal(pos_u, ref[name][a:b]) and np.array_equal(_bits(mx_u), _bits(mx)), (i, name)
        # the schedule itself, as read off PrunePolicy: pruned, pruned, kPruneProbeEvery dense calls, the probe, pruned
        assert forms == [True, True] + [False] * policy.probe_every + [True, True], forms
        print(f"prune interleaved: {len(calls)} calls, {forms.count(True)} pruned, {forms.count(False)} dense and folded, "
              f"kept {kept} of {total}; D {cnt['D']}, Q {cnt['Q']}; {time.perf_counter() - t0:.2f} s")
    finally:
        main.close()
        unfolded.close()
