"""The scenes of tests/test_gpu_exact_lengths.py are hard — shown without a GPU, on the restatements alone.

For every Set the GPU file runs (exact_scenes.used_sets: one FP32 order, kernel length, window shape, content and sign each) two
things are computed, through the table both files read (exact_scenes.evaluate): the float32 emulation of the family's operation
order (fp32_restatement.response_of_order with the DC level dc_level decides) and the dense Float64 oracle's position.  Then:
  * every hard family the Set was built with (0 ... 3 and 5) is present, and local-dc windows inside the frame sample a DC level
    that is not the fill;
  * the emulated FP32 argmax (first in column-major order) differs from the oracle's position on at least one window, and on at
    least 3 % of the windows of a Set of 64 or more: on these windows a kernel that only ranks its FP32 responses answers wrongly,
    so the GPU census is not vacuous;
  * on every window of families 0, 1 and 3 the emulated map's two best responses (the second: the largest of any OTHER pixel) lie
    within threshold_f32(F) V / 255, F = factor(order, g+, g-), V = max|pixel - dc| over the tile: windows the flag must catch;
  * the control family 4 is ranked correctly everywhere: a scene bug does not pass for a hard window.
These are conditions on the inputs, not measurements of a kernel.  A noise-only window meets the flag rule with its own V only
by chance (1 draw in 2 at l = 149, 1 in 700 at l = 17), and a one-level disc never: so family 1's target has an even diameter
(four tied pixels) and the noise of families 0 and 1 is drawn until the emulation meets the rule — and, for the first window of
the chains' noise-only sets, until FP32 also misranks.  exact_scenes.search_attempts finds the draws,
tests/golden/exact_scene_attempts.json records them, and this file checks every one of them.
Every Set prints one `scenes` line with the shares (profiles/exact_lengths_census.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_scenes as xs  # noqa: E402


def _sets():
    from oracle.dog_oracle import Oracle, build
    build()
    return xs.used_sets(Oracle())


SETS = _sets()


def test_the_sets_cover_the_issue_s_cases():
    kinds = {(S.order, S.l) for S in SETS}
    assert {("roll", l) for l in (17, 29, 49, 65, 81, 101, 109, 125, 149)} <= kinds
    assert {("fused", l) for l in (29, 45, 65, 85, 101)} | {("tiled", l) for l in (29, 65, 101)} | {("ring", 29), ("ring", 65)} <= kinds
    assert {("twopass", l) for l in (29, 65, 101, 113, 125, 293)} <= kinds
    assert any(S.content == "local dc" for S in SETS) and any(not S.darker for S in SETS)
    assert len(SETS) == len(set(SETS))


@pytest.mark.parametrize("S", SETS, ids=xs.label)
def test_the_scenes_are_hard(oracle, S):
    ev = xs.evaluate(oracle, S, emulate=True)
    fam, dense, emu = ev["fam"], ev["dense"], ev["emu"]
    n = len(fam)
    assert n == S.n and n >= len(S.families) and set(fam.tolist()) == set(S.families)
    if S.content == "local dc":
        inner = fam != 5
        assert inner.any() and (ev["dc"][inner] != ev["fills"][inner]).all(), ev["dc"]
    wrong = (emu != dense).any(1)
    flagged = ev["gap"] <= ev["bound"]
    must = np.isin(fam, (0, 1, 3))
    per_family = {f: f"{int(wrong[fam == f].sum())}/{int((fam == f).sum())}" for f in sorted(set(fam.tolist()))}
    print(f"scenes {xs.label(S)} seed={ev['seed']}: FP32 ranking alone differs from the dense oracle on {int(wrong.sum())} of {n} windows "
          f"({100.0 * wrong.mean():.1f} %; per family {per_family}); under the flag rule {int(flagged.sum())} of {n}, "
          f"families 0/1/3 {int((flagged & must).sum())} of {int(must.sum())}; T={ev['T']:.3e} V={int(ev['V'].min())}..{int(ev['V'].max())}")
    assert wrong.sum() >= 1, "no window of the set is decided by the Float64 arithmetic"
    if n >= 64:
        assert wrong.mean() >= 0.03, wrong.mean()
    bad = np.flatnonzero(must & ~flagged)
    assert bad.size == 0, (bad.tolist(), fam[bad].tolist(), ev["gap"][bad].tolist(), ev["bound"][bad].tolist())
    easy = fam == 4
    assert not wrong[easy].any(), np.flatnonzero(wrong & easy).tolist()
