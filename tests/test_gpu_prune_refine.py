"""The pre-pass's second stage on the GPU (csrc/dog_prune.hpp, "the cell bound") against its NumPy restatement
(tests/prune_refine_restatement.py) on the scenes of tests/prune_refine_scenes.py — l = 17, 65, 109; one strip, strips with a
remainder column, a shifted second strip; windows over the frame's corner, a disc on the strips' boundary, two equal discs, bright
targets, ±3 and ±40 levels, flat and noise-only windows (tests/test_prune_refine_cpu.py shows what the restatement does there).

Per set, with default tuning, `no_refine` = 1 and `no_prune` = 1, exact mode on, the roll variant pinned:
  * positions equal the dense Float64 oracle's in all three;
  * batch_maxima() bit-equal across the three;
  * exact_stats()[2] advances equally;
  * prune_counts() is the FIRST stage's (kept, total) of tests/prune_restatement.py in both pruned modes, (0, 0) under `no_prune`;
  * prune_jobs(), sorted, equals the restatement's refined non-empty strip ranges entry for entry by default and the first
    stage's hulls under `no_refine`.
A fresh tracker per mode: the pruning policy decides on the first stage's share, which on several of these small sets lies above
its break-even, so a second batch on the same tracker would run dense (csrc/pdog_policy.hpp).
test_fenced_publish: the same with `fenced_publish` = 1.  test_frame_edges_and_strided_table: the 83-column frames and the
strided frame table of tests/test_gpu_prepass_edges.py, window by window.
Measured on an MI355X: the file's 9 tests together 2.7 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_refine_restatement as rr  # noqa: E402
import prune_refine_scenes as scenes  # noqa: E402
import prune_length_scenes as ps  # noqa: E402
import test_gpu_prepass_edges as edges  # noqa: E402

pytestmark = pytest.mark.gpu
SETS = scenes.sets()
MODES = (("default", {}), ("no_refine", {"no_refine": 1}), ("no_prune", {"no_prune": 1}))


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_REF = {}


def _oracle_positions(oracle, st):
    if st.name not in _REF:
        sg = oracle.sigma(st.tw)
        _REF[st.name] = oracle.detect_batch_par(st.frames(), st.fill, oracle.dog_kernel(sg, st.darker), sg, st.darker, st.radii, st.guesses(), separable=False)
    return _REF[st.name]


def _run(pt, st, **tuning):
    """(positions, maxima, windows re-evaluated, prune_counts, sorted jobs or None) of the set as one batch on a fresh tracker."""
    import torch
    bt = pt.BatchTracker(st.fh, st.fw, st.tw, st.ws, st.darker, st.fill)
    try:
        assert bt.info().kernel_len == st.l
        bt.set_variant(ps.variant_id(st.l))
        for key, value in tuning.items():
            bt.set_tuning(key, value)
        bt.set_exact(1)
        frames, guesses = st.frames(), st.guesses()
        assert bt.kernel_for_batch(len(frames)) == ps.variant_id(st.l)
        pos = bt.detect(torch.from_numpy(frames).cuda(), torch.from_numpy(guesses).cuda())
        bt.sync()
        jobs = None if tuning.get("no_prune") else sorted(tuple(int(v) for v in row) for row in bt.prune_jobs())
        return pos.cpu().numpy(), bt.batch_maxima(len(frames)), bt.exact_stats()[2], bt.prune_counts(), jobs
    finally:
        bt.close()


def _three_modes(pt, oracle, st, **extra):
    ref = _oracle_positions(oracle, st)
    want_counts = st.counts()
    res = {name: _run(pt, st, **tuning, **extra) for name, tuning in MODES}
    for name, (pos, mx, refined, counts, jobs) in res.items():
        print(f"{st.name} {name}: counts {counts} (restatement {want_counts}), {None if jobs is None else len(jobs)} jobs "
              f"(restatement: refined {len(st.jobs(True))}, first stage {len(st.jobs(False))}), re-evaluated {refined}")
    for name, (pos, mx, refined, counts, jobs) in res.items():
        assert np.array_equal(pos, ref), (st.name, name, np.argwhere(pos != ref)[:4])
        assert np.array_equal(_bits(mx), _bits(res["no_prune"][1])), (st.name, name)
        assert refined == res["no_prune"][2], (st.name, name)
        assert counts == ((0, 0) if name == "no_prune" else want_counts), (st.name, name, counts, want_counts)
    assert res["default"][4] == st.jobs(True), (st.name, [a for a in zip(res["default"][4], st.jobs(True)) if a[0] != a[1]][:4])
    assert res["no_refine"][4] == st.jobs(False), (st.name, [a for a in zip(res["no_refine"][4], st.jobs(False)) if a[0] != a[1]][:4])
    assert st.jobs(True) != st.jobs(False)


@pytest.mark.parametrize("st", SETS, ids=[s.name for s in SETS])
def test_refined_ranges_are_the_restatements(pt, oracle, st):
    _three_modes(pt, oracle, st)


def test_fenced_publish(pt, oracle):
    _three_modes(pt, oracle, next(s for s in SETS if s.name == "l65-strips-remainder"), fenced_publish=1)


@pytest.mark.parametrize("vid,l,shape,fh", edges.CONFIGS)
def test_frame_edges_and_strided_table(pt, oracle, vid, l, shape, fh):
    """Tiles over every edge of an 83-column frame, the frames at the odd places of a strided stack with a frame table: the
    refined range of every window, each as a batch of its own, and the position."""
    frames, guesses, origins, ref, counts = edges._case(oracle, l, shape, fh)
    import torch
    tw, radii = edges._tw_for_kernel_len(l), (shape[0] // 2, shape[1] // 2)
    nstrips = len([1 for _, w in pr.slots(shape[1]) if w > 1])
    d_f, d_idx = edges._stack(frames, 255)
    d_g = torch.from_numpy(guesses).cuda()
    narrowed = 0
    for k in range(len(frames)):
        tile = fr.window_tile(frames[k], edges.FILL, l, radii, guesses[k])
        pp = pr.prepass(tile, edges.FILL, tw, True)
        rf = rr.refine(tile, edges.FILL, tw, True, pp)
        want = sorted((0, s, ba, bb) for s, (ba, bb) in enumerate(rf["hull"][:nstrips]) if bb > ba)
        narrowed += rf["hull"] != pp["hull"]
        bt = edges._tracker(pt, vid, l, shape, fh, 0, 1)
        try:
            pos = bt.detect(d_f, d_g[k:k + 1].contiguous(), frame_index=d_idx[k:k + 1].contiguous())
            bt.sync()
            got = sorted(tuple(int(v) for v in row) for row in bt.prune_jobs())
            kc = bt.prune_counts()
            pos = pos.cpu().numpy()
        finally:
            bt.close()
        assert kc == counts[k], (k, origins[k], kc, counts[k])
        assert got == want, (k, origins[k], got, want, pp["hull"])
        assert np.array_equal(pos[0], ref[k]), (k, origins[k], pos[0], ref[k])
    assert narrowed > 0
