"""tests/prune_length_scenes.py shown to hold what tests/test_gpu_prune_lengths.py relies on, with the NumPy restatement of the
pre-pass (tests/prune_restatement.py) alone, for all 34 roll kernel lengths and both target signs:
  * every class of kept range in prune_length_scenes.CLASSES occurs in the ten windows of a length;
  * every window prunes (kept < total), and the window that holds a disc of either sign keeps another number of pairs when
    the sign of the 3 × 3-cell sums is flipped — so the kernel's counts tell a wrong PruneGeo::darker;
and, for bright targets, which tests/test_prune_cpu.py never ran — every scene at l = 17, 65, 109, 149 — against the float32
emulation of the roll order (tests/fp32_restatement.py):
  * L is at most the emulated map's maximum;
  * no pixel outside the hulls lies within T_max of the maximum;
  * the maximum's own block is kept.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_length_scenes as ps  # noqa: E402


@pytest.mark.parametrize("darker", (True, False), ids=("dark", "bright"))
@pytest.mark.parametrize("l", ps.LENGTHS)
def test_every_class_of_kept_range_occurs(l, darker):
    tw = ps.tw_for_kernel_len(l)
    assert fr.kernel_len(fr.sigma_of(tw)) == l
    frames, guesses, fill = ps.scenes(l, darker)
    n1, n2 = ps.geometry(l)[1]
    assert 8 <= len(frames) <= 12 and n1 % 2 == 1 and n2 == 131
    assert n1 * n2 * l * l * len(frames) < 1e10                      # the dense oracle's budget per length
    pps = ps.restate(l, darker, frames, guesses, fill)
    found = ps.classes_of(l, pps)
    for c in ps.CLASSES:
        print(f"l={l} {'dark' if darker else 'bright'} {c}: {found[c][:3]}")
    missing = [c for c in ps.CLASSES if not found[c]]
    assert not missing, (l, darker, missing, [pp["hull"] for pp in pps])
    for w, (kept, total) in enumerate(ps.counts(l, pps)):
        assert 0 < kept < total, (l, darker, w, kept, total)
    # the window with a disc of either sign: the cell sums signed the wrong way lead L to the other disc
    tile = ps.tiles(l, frames, guesses, fill)[ps.TWO_SIGN]
    right = pr.kept_pairs(pps[ps.TWO_SIGN], l)
    wrong = pr.kept_pairs(pr.prepass(tile, fill, tw, darker, cell_darker=not darker), l)
    print(f"l={l} two-sign window: kept {right[0]} of {right[1]}, with the cell sign flipped {wrong[0]}")
    assert right[0] != wrong[0] and right[1] == wrong[1], (l, darker, right, wrong)


def test_geometry_constants_follow_the_headers():
    """roll_prologue_len and the phase count as csrc/dog_roll.hpp's comments state them at both ends, and the lengths
    are roll_lengths.def's."""
    assert (ps.roll_prologue_len(17), ps.roll_prologue_len(65), ps.roll_prologue_len(149)) == (2, 8, 18)
    assert (ps.roll_phases(17), ps.roll_phases(65), ps.roll_phases(149)) == (3, 9, 20)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import re
    text = open(os.path.join(root, "pawsometracker.jl_amd", "csrc", "roll_lengths.def")).read()
    listed = [int(m) for m in re.findall(r"PDOG_ROLL_L\((\d+)\)", text)]
    assert listed == list(ps.LENGTHS), listed


@pytest.mark.parametrize("l", (17, 65, 109, 149))
def test_bright_targets_lower_bound_and_hull(l):
    darker = False
    tw = ps.tw_for_kernel_len(l)
    frames, guesses, fill = ps.scenes(l, darker)
    for w, tile in enumerate(ps.tiles(l, frames, guesses, fill)):
        resp = fr.response_f32(tile, fill, tw, darker, "roll")
        pp = pr.prepass(tile, fill, tw, darker)
        M = float(resp.max())
        (oy, ox), blk = pp["origin"], 8
        assert np.float32(pp["L"]).view(np.int32) == resp[oy:oy + blk, ox:ox + blk].max().view(np.int32), (l, w)
        assert pp["L"] <= M, (l, w)
        my, mx = np.unravel_index(int(np.argmax(resp)), resp.shape)
        for s, (c0, width) in enumerate(pp["slots"]):
            ba, bb = pp["hull"][s]
            near = np.argwhere(resp[:, c0:c0 + width].astype(np.float64) >= M - pp["Tmax"])
            for y, _ in near:
                assert 8 * ba <= y < 8 * bb, (l, w, s, int(y), (ba, bb))
            if c0 <= mx < c0 + width:
                assert ba <= my // 8 < bb, (l, w, s, (my, mx), (ba, bb))
