"""The scenes the blob rule (include/pawsome_blob.h) is tested on beside those of tests/shape_scenes.py, as calls:
  (a) diagonal touch: two 5 x 5 squares that share only a corner — 50 pixels under connectivity 8, 25 under 4;
  (b) seed tie: the centre pixel at background, the (-1, -1) and (+1, +1) pixels equally dark, each on a blob of its own (25
      and 49 pixels) that the other does not touch — the row-major-first pixel, (-1, -1), is the seed;
  (c) long geodesics at R = 12, 31, 32 and 127 (the last on 260 x 260): a vertical comb, a horizontal comb (serpentines of
      pitch 2) and a square spiral corridor of pitch 2, each inside the square inscribed in the disc — a mask cannot hold half
      the patch or more, its pixels lie strictly on one side of the median —, one position each;
  (d) binary {40, 128} noise, the 3 x 3 under the position forced dark, one position for EVERY radius 2 ... 127, at the site
      percolation densities 0.60 (connectivity 4) and 0.42 (connectivity 8): on 260 x 260 with the patch inside the frame, and
      on 120 x 160 under fill 128 and fill 40, where the patch overhangs the frame's upper edge and, under fill 40, the padding
      is mask and the blob runs through it.  At density 0.60 the dark pixels are the patch's majority, so the median is dark
      and the rule's mask is EMPTY (the case is kept as a call all the same); connectivity 4 therefore also runs at 0.47, the
      nearest density at which the dark pixels stay the minority in nearly every patch;
  (e) a bar through the whole patch: n_rim > 0.
`cases()` lists them with shape_scenes' Case plus the connectivities a case is meant for; `reference(case, connectivity)` is the
restatement's answer, computed once.  TEST HELPER: nothing here loads the library under test."""
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blob_restatement as BLR  # noqa: E402
import shape_restatement as SR  # noqa: E402

H, W = 120, 160
BIG = 260
DARK, FLOOR = 40, 128
GEODESIC_RADII = (12, 31, 32, 127)
NOISE_RADII = tuple(range(2, 128))

# as shape_scenes.Case, and conns: the connectivities the case is run with
Case = namedtuple("Case", "name frames ij fi radius fill darker min_contrast tw conns")


def _case(name, frame, ij, radius, fill=FLOOR, conns=(4, 8), fi=None):
    frames = frame[None] if frame.ndim == 2 else frame
    ij = np.array(ij, np.int32).reshape(-1, 2)
    fi = np.zeros(len(ij), np.int32) if fi is None else np.asarray(fi, np.int32)
    return Case(name, frames, ij, fi, radius, fill, True, 8, 25.0, conns)


def diagonal_touch():
    f = np.full((H, W), FLOOR, np.uint8)
    f[56:61, 76:81] = DARK           # centre (58, 78), 0-based
    f[61:66, 81:86] = DARK           # shares the corner (60, 80) | (61, 81) only
    return _case("diagonal touch", f, [(59, 79)], 12)


def seed_tie():
    f = np.full((H, W), FLOOR, np.uint8)
    f[54:59, 74:79] = DARK           # 25 pixels, ends in (58, 78): (-1, -1) of the position (59, 79), 0-based
    f[60:67, 80:87] = DARK           # 49 pixels, starts in (60, 80): (+1, +1)
    return _case("seed tie", f, [(60, 80)], 12)


def _half_side(R):
    return int(math.floor(R / math.sqrt(2.0))) - 1


def comb_mask(R, vertical):
    """A serpentine of pitch 2 in the square |y|, |x| <= q: corridors along every second column (vertical) or row, joined at
    alternating ends.  bool [D, D]."""
    q = _half_side(R)
    q -= q % 2                                   # corridors at the even offsets -q ... q, the centre's among them
    D = 2 * R + 1
    m = np.zeros((D, D), bool)
    for k, x in enumerate(range(-q, q + 1, 2)):
        m[R - q:R + q + 1, R + x] = True
        if x + 2 <= q:
            m[R + (q if k % 2 == 0 else -q), R + x + 1] = True
    return m if vertical else m.T.copy()


def spiral_mask(R):
    """A square spiral corridor of pitch 2 (one pixel of corridor, one of wall) from the centre outwards, inside |y|, |x| <= q."""
    q = _half_side(R)
    D = 2 * R + 1
    m = np.zeros((D, D), bool)
    y = x = 0
    m[R, R] = True
    step, d = 2, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for _ in range(2):
            ey, ex = dirs[d % 4]
            for _ in range(step):
                y, x = y + ey, x + ex
                if max(abs(y), abs(x)) > q:
                    return m
                m[R + y, R + x] = True
            d += 1
        step += 2


def geodesic(R, kind):
    h, w = (BIG, BIG) if R == 127 else (H, W)
    f = np.full((h, w), FLOOR, np.uint8)
    ci, cj = h // 2, w // 2                       # 0-based centre; the patch lies inside the frame
    m = {"vertical comb": lambda: comb_mask(R, True), "horizontal comb": lambda: comb_mask(R, False), "spiral": lambda: spiral_mask(R)}[kind]()
    box = f[ci - R:ci + R + 1, cj - R:cj + R + 1]
    box[m] = DARK
    return _case(f"{kind} R {R}", f, [(ci + 1, cj + 1)], R)


def _noise_frame(h, w, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, DARK, FLOOR).astype(np.uint8)


NOISE_DENSITIES = ((0.60, (4,)), (0.42, (8,)), (0.47, (4,)))


def noise_inside(density, conns):
    """260 x 260, every radius at the frame's centre: the patch inside the frame."""
    f = _noise_frame(BIG, BIG, density, [11, int(density * 100)])
    f[129:132, 129:132] = DARK
    return [_case(f"noise {density:.2f} inside R {R}", f, [(131, 131)], R, conns=conns) for R in NOISE_RADII]


def noise_overhang(density, conns, fill):
    """120 x 160, radius R at row R + 1 - R // 4 (1-based): the patch overhangs the upper edge by R // 4 rows — and, from R = 60
    on, the lower edge too."""
    f = _noise_frame(H, W, density, [12, int(density * 100)])
    out = []
    for R in NOISE_RADII:
        i = min(R + 1 - R // 4, H - 1)
        g = f.copy()
        g[i - 2:i + 1, 79:82] = DARK
        out.append(_case(f"noise {density:.2f} fill {fill} R {R}", g, [(i, 81)], R, fill=fill, conns=conns))
    return out


def bar():
    f = np.full((H, W), FLOOR, np.uint8)
    f[57:62, :] = DARK                            # five rows through the whole frame
    return _case("bar", f, [(60, 80)], 25)


_CASES = None
_REF = {}


def cases():
    global _CASES
    if _CASES is None:
        c = [diagonal_touch(), seed_tie(), bar()]
        c += [geodesic(R, kind) for R in GEODESIC_RADII for kind in ("vertical comb", "horizontal comb", "spiral")]
        _CASES = c
    return _CASES


_NOISE = None


def noise_cases():
    """The noise scenes, one case per radius: a list of (group name, [Case ...])."""
    global _NOISE
    if _NOISE is None:
        g = []
        for density, conns in NOISE_DENSITIES:
            g.append((f"inside {density:.2f}", noise_inside(density, conns)))
            for fill in (FLOOR, DARK):
                g.append((f"overhang {density:.2f} fill {fill}", noise_overhang(density, conns, fill)))
        _NOISE = g
    return _NOISE


def case(name):
    return next(c for c in cases() if c.name == name)


def reference(c, connectivity):
    """(shape [n, 6] float64, sums [n, 10] int32) of the restatement for a case (of this file or of shape_scenes) and a
    connectivity, computed once and read-only."""
    key = (c.name, connectivity)
    if key not in _REF:
        R = c.radius or SR.default_radius(c.tw)
        shp, words = BLR.blobs(c.frames, c.ij, c.fi, R, c.fill, c.darker, c.min_contrast, connectivity)
        shp.setflags(write=False)
        words.setflags(write=False)
        _REF[key] = (shp, words)
    return _REF[key]
