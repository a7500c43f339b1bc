"""The scenes the split rule (include/pawsome_split.h) is tested on, as calls of ONE set each unless said otherwise:
  (a) ellipses with semi-axes (12, 5) at value 30 on shape_scenes.floor_frame, overlapping animals combined by the maximum of
      their coverages, the positions the rounded centres + 1, R = 25: "side by side" (parallel, 9.4 px apart), "T" (head
      against flank), "head to tail" (collinear, 23 px apart), "apart", and "three" (two touching, one 23 px away); ALONE[name]
      holds every animal of a scene on a frame of its own (the same floor);
  (b) ties: a rival on the same pixel; rivals at (0, +6) and (+4, +4) on a dark square, tie pixels on both bisectors (R = 25);
      a rival at exactly (0, 2R) and one at (0, 2R + 1) on a bar through the patch (R = 12);
  (c) 32 targets within R of one another on noise;
  (d) every radius 2 ... 127: three targets on blob_scenes' 260 x 260 noise frames at (131, 131), (131 + R // 2, 131 - R // 3)
      and (131 - R, 131 + R // 4), connectivity 8 at density 0.42 and 4 at 0.47 — radius_cases();
  (e) the tier boundary: R = 31, 32 and 127 with six targets;
  (f) overhang: the patch over the frame's upper edge under fill 128 and fill 40, one rival given outside the frame (clamped);
  (g) bright targets: "side by side" inverted, darker = False;
  (h) "stack": the four two-animal ellipse scenes as four sets on four frames.
`cases()` lists all but (d); `reference(case, connectivity)` is the restatement's answer, computed once.  TEST HELPER: nothing
here loads the library under test."""
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blob_scenes as BLS  # noqa: E402
import shape_scenes as SS  # noqa: E402
import split_restatement as SPR  # noqa: E402

H, W = SS.H, SS.W
A, B, VALUE, R_ELL = 12, 5, 30, 25
FLOOR_SEED = 2024

# frames uint8 [nf, h, w]; ij int32 [n_sets, n_targets, 2] 1-based; set s looks at frame s
Case = namedtuple("Case", "name frames ij radius fill darker min_contrast conns")


def _c20(d):
    return d * math.cos(math.radians(20)), -d * math.sin(math.radians(20))


# name: [(cy, cx, degrees) ...], 0-based centres as shape_scenes.coverage takes them
ELLIPSES = {
    "side by side": [(55.3, 70.6, 20), (55.3 + _c20(9.4)[0], 70.6 + _c20(9.4)[1], 20)],
    "T": [(50.2, 80.4, 0), (66.7, 83.4, 90)],
    "head to tail": [(60.2, 60.4, 10), (60.2 + 23 * math.sin(math.radians(10)), 60.4 + 23 * math.cos(math.radians(10)), 10)],
    "apart": [(40.2, 40.4, 10), (80.2, 110.4, 60)],
    "three": [(55.3, 70.6, 0), (64.6, 70.9, 0), (60.0, 94.0, 90)],
}
TOUCHING = {"side by side": (0, 1), "T": (0, 1), "head to tail": (0, 1), "apart": (), "three": (0, 1)}


def animals_frame(animals):
    """The animals at value VALUE on the floor, overlapping ones combined by the maximum of their coverages."""
    cov = np.zeros((H, W))
    for cy, cx, deg in animals:
        cov = np.maximum(cov, SS.coverage(cy, cx, A, B, deg))
    f = SS.floor_frame(FLOOR_SEED) * (1.0 - cov) + VALUE * cov
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def positions_of(animals):
    return np.array([(int(round(cy)) + 1, int(round(cx)) + 1) for cy, cx, _ in animals], np.int32)


def _ellipse_case(name):
    an = ELLIPSES[name]
    return Case(name, animals_frame(an)[None], positions_of(an)[None], R_ELL, 128, True, 8, (4, 8))


def alone(name, k):
    """(frame, position) of animal k of an ellipse scene without the others."""
    an = ELLIPSES[name]
    return animals_frame([an[k]]), positions_of(an)[k]


def _tie_cases():
    sq = np.full((H, W), BLS.FLOOR, np.uint8)
    sq[45:75, 65:95] = BLS.DARK                   # 30 x 30 around (60, 80), 1-based
    bar = BLS.bar().frames[0]
    R = 12                                        # (the square is the minority of a patch of R = 25 only: the median stays floor)
    return [Case("same pixel", sq[None], np.array([[(60, 80), (60, 80)]], np.int32), 25, 128, True, 8, (4, 8)),
            Case("bisector ties", sq[None], np.array([[(58, 76), (58, 82), (62, 80)]], np.int32), 25, 128, True, 8, (4, 8)),
            Case("rival at 2R", bar[None], np.array([[(60, 60), (60, 60 + 2 * R)]], np.int32), R, 128, True, 8, (4, 8)),
            Case("rival at 2R + 1", bar[None], np.array([[(60, 60), (60, 61 + 2 * R)]], np.int32), R, 128, True, 8, (4, 8))]


def _noise(density):
    return BLS.noise_inside(density, (8,))[0].frames[0]


def _cluster_case():
    rng = np.random.default_rng(32)
    f = BLS._noise_frame(BLS.BIG, BLS.BIG, 0.30, [13, 30])      # (sparser: the 32 forced 3 x 3 stay the patch's minority)
    ij = np.stack([131 + rng.integers(-12, 13, 32), 131 + rng.integers(-12, 13, 32)], 1).astype(np.int32)      # within 25 of one another ... nearly
    ij[31] = ij[3]                                   # and two on one pixel
    for i, j in ij:
        f[i - 2:i + 1, j - 2:j + 1] = BLS.DARK
    return Case("32 targets", f[None], ij[None], 25, 128, True, 8, (4, 8))


def radius_positions(R):
    return np.array([[(131, 131), (131 + R // 2, 131 - R // 3), (131 - R, 131 + R // 4)]], np.int32)


def radius_cases(connectivity):
    """(d): one case per radius 2 ... 127 for the connectivity, all on one frame."""
    f = _noise(0.42 if connectivity == 8 else 0.47)[None]
    return [Case(f"radius {R} conn {connectivity}", f, radius_positions(R), R, 128, True, 8, (connectivity,)) for R in BLS.NOISE_RADII]


def _tier_cases():
    f = _noise(0.42)[None]
    out = []
    for R in (31, 32, 127):
        ij = np.array([[(131, 131), (131, 131 + R // 3), (131 - R // 2, 131 - R // 2), (131 + R, 131 - 3), (131 + 2, 131 - 2 * R), (131 + 2 * R + 1, 131)]], np.int32)
        out.append(Case(f"tier R {R}", f, ij, R, 128, True, 8, (4, 8)))
    return out


def _overhang_cases():
    out = []
    for fill in (BLS.FLOOR, BLS.DARK):
        c = dict(BLS.noise_cases())[f"overhang 0.42 fill {fill}"][25 - 2]       # R = 25, position (20, 81)
        assert c.radius == 25 and tuple(c.ij[0]) == (20, 81)
        ij = np.array([[(20, 81), (-5, 90), (25, 70)]], np.int32)               # the second is clamped to (1, 90)
        out.append(Case(f"overhang fill {fill}", c.frames, ij, 25, fill, True, 8, (4, 8)))
    return out


def _bright_case():
    c = _ellipse_case("side by side")
    return Case("bright side by side", 255 - c.frames, c.ij, R_ELL, 128, False, 8, (4, 8))


def _stack_case():
    names = ("side by side", "T", "head to tail", "apart")
    return Case("stack", np.concatenate([_ellipse_case(n).frames for n in names]), np.concatenate([_ellipse_case(n).ij for n in names]),
                R_ELL, 128, True, 8, (8,))


_CASES = None
_REF = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = ([_ellipse_case(n) for n in ELLIPSES] + _tie_cases() + [_cluster_case()] + _tier_cases() + _overhang_cases()
                  + [_bright_case(), _stack_case()])
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def reference(c, connectivity):
    """(shape [n_sets, n_targets, 6] float64, sums [n_sets, n_targets, 12] int32) of the restatement, computed once, read-only."""
    key = (c.name, connectivity)
    if key not in _REF:
        shp, words = SPR.split_blobs(c.frames, c.ij, None, c.radius, c.fill, c.darker, c.min_contrast, connectivity)
        shp.setflags(write=False)
        words.setflags(write=False)
        _REF[key] = (shp, words)
    return _REF[key]
