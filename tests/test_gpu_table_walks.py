"""The table walks back to back on ONE tracker and one stream, with no synchronisation in between: an indexed walk, an exclusive
walk, a motion walk, a predicted walk on a one-launch path, a predicted walk that falls back to the motion walk (a table of one
step), and the indexed walk again — every family stages its table through the same type (csrc/pdog_host.hpp, StagedTable), and a
walk that overwrote words another still reads, or a length vector of the wrong family, would show here.  Every result equals,
bit for bit, the same call on a fresh tracker that is synchronised behind it; a second round leaves every `grown` as it was."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exclusive_scenes as es  # noqa: E402

pytestmark = pytest.mark.gpu
WS = 41                      # tests/test_gpu_exclusive.py's window
G, T, NF = 2, 3, 10
FULL, ONE, NONE = list(range(NF)), [3] + [-1] * (NF - 1), [-1] * NF


def test_back_to_back_walks_equal_fresh_trackers():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import pawsometracker_jl_amd as pt
    sc = es.scene("through")
    d_frames = torch.from_numpy(np.ascontiguousarray(sc.frames[:NF])).cuda()
    jit = np.random.default_rng(3).integers(-6, 7, (G, T, 2))
    jit[:, :2] = 0                                              # two targets on the discs, a third beside one of them
    starts = (np.array([[sc.truth[0][t % 2] for t in range(T)]] * G) + jit).astype(np.int32)
    d_groups, d_clips = torch.from_numpy(starts).cuda(), torch.from_numpy(starts.reshape(G * T, 2)).cuda()
    clips = np.array([FULL, ONE, NONE, FULL[::-1], ONE, FULL], np.int32)          # rows of 0, 1 and all steps
    one_step = np.array([[2], [5], [-1], [0], [9], [7]], np.int32)
    calls = [
        ("indexed", lambda bt: (bt.detect_chains_indexed(d_frames, clips, d_clips),)),
        ("exclusive", lambda bt: bt.detect_chains_exclusive(d_frames, np.array([FULL, ONE], np.int32), d_groups)),
        ("motion", lambda bt: bt.detect_chains_motion(d_frames, np.array([NONE, FULL], np.int32), d_groups, first=1)),
        ("predicted", lambda bt: bt.detect_chains_predicted(d_frames, clips, d_clips)),
        ("fallback", lambda bt: bt.detect_chains_predicted(d_frames, one_step, d_clips)),
        ("indexed", lambda bt: (bt.detect_chains_indexed(d_frames, clips, d_clips, first=1),)),
    ]
    make = lambda: pt.BatchTracker(es.H, es.W, es.TW, (WS, WS), True, es.BKGD)

    want = []
    for _, call in calls:
        fresh = make()
        try:
            want.append(call(fresh))
            fresh.sync()
        finally:
            fresh.close()
    assert int(want[0][0].abs().sum()) > 0 and int(want[1][1].abs().sum()) > 0 and int(want[2][1].abs().sum()) > 0   # the walks did walk

    bt = make()
    try:
        grown = lambda: (bt.exclusive_counts()[1], bt.motion_counts()[1], bt.predict_counts()[3])
        for rnd in range(2):
            before = bt.predict_counts()
            got = [call(bt) for _, call in calls]                # nothing waits in between
            bt.sync()
            moved = [a - b for a, b in zip(bt.predict_counts(), before)]
            assert moved[0] + moved[1] == 1 and moved[2] == 1, moved      # one walk in one launch, one handed to the motion walk
            for (name, _), g, w in zip(calls, got, want):
                assert len(g) == len(w) and all(torch.equal(a, b) for a, b in zip(g, w)), (rnd, name)
            if rnd == 0:
                first_round = grown()
                assert all(v > 0 for v in first_round), first_round
        assert grown() == first_round
    finally:
        bt.close()
