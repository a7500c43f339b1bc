"""The scenes the shape rule (include/pawsome_shape.h) is tested on, all 120 x 160:
  (a) filled ellipses drawn by 4 x 4 supersampled coverage on the floor 100 + floor(0.3 * col) under +-2 seeded noise, value 40
      (dark) and 220 (bright), semi-axes (12, 5) at R = 25 and (6, 3) at R = 12, 36 angles in 5 degree steps, sub-pixel centres,
      measured at the centre pixel and at two positions one pixel off;
  (b) the reference's own disc recipe (oracle.synth.disc_frame, tw 10 and 25) at the centre and 3 px off it;
  (c) an ellipse that moves along its long axis, then stops, then reverses (for the headings);
  (d) degenerate cases: a flat frame, a position on empty noisy floor, a disc at the frame's corner with most of the patch
      outside the frame (under a fill far from the floor), and a second, darker object inside the patch — the rule's known
      limit, shown, not hidden.
`cases()` lists them as calls: frames, positions, frame index and the call's parameters; `reference(case)` is the restatement's
answer, computed once.  TEST HELPER: nothing here loads the library under test."""
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shape_restatement as SR  # noqa: E402
from oracle import synth  # noqa: E402

H, W = 120, 160
ANGLES = [5 * k for k in range(36)]          # degrees, from +col towards +row

# frames uint8 [nf, H, W]; ij int32 [n, 2] 1-based; fi int32 [n]; tw: the tracker's target_width (its default radius);
# truth: per position None or (row, col, angle in degrees or None, major, minor), 1-based
Case = namedtuple("Case", "name frames ij fi radius fill darker min_contrast tw truth")


def floor_frame(seed):
    rng = np.random.default_rng(seed)
    base = 100 + np.floor(0.3 * np.arange(W)).astype(np.int64)
    return np.broadcast_to(base, (H, W)) + rng.integers(-2, 3, (H, W))


def coverage(cy, cx, a, b, deg):
    """The share of every pixel (a unit square around its 0-based centre) inside the ellipse with centre (cy, cx), semi-axes
    a (along the angle) and b: 4 x 4 samples per pixel."""
    phi = math.radians(deg)
    off = (np.arange(4) + 0.5) / 4 - 0.5
    y = (np.arange(H)[:, None] + off[None, :]).reshape(-1)[:, None] - cy
    x = (np.arange(W)[:, None] + off[None, :]).reshape(-1)[None, :] - cx
    u = x * math.cos(phi) + y * math.sin(phi)
    v = -x * math.sin(phi) + y * math.cos(phi)
    inside = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    return inside.reshape(H, 4, W, 4).mean(axis=(1, 3))


def ellipse_frame(cy, cx, a, b, deg, value, seed):
    cov = coverage(cy, cx, a, b, deg)
    f = floor_frame(seed) * (1.0 - cov) + value * cov
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _ellipse_case(a, b, R, value):
    frames, ij, fi, truth = [], [], [], []
    for k, deg in enumerate(ANGLES):
        cy, cx = 58.0 + (k * 0.37) % 1.0, 80.0 + (k * 0.61) % 1.0
        frames.append(ellipse_frame(cy, cx, a, b, deg, value, [a, b, value, k]))
        i, j = int(round(cy)) + 1, int(round(cx)) + 1
        for p in ((i, j), (i + 1, j), (i, j - 1)):
            ij.append(p)
            fi.append(k)
            truth.append((cy + 1, cx + 1, deg, 2.0 * a, 2.0 * b))
    dark = value < 100
    return Case(f"ellipse ({a}, {b}) R {R} {'dark' if dark else 'bright'}", np.stack(frames), np.array(ij, np.int32),
                np.array(fi, np.int32), R, 128, dark, 8, float(R), truth)


def _disc_case(tw, darker):
    c = (61, 83)
    frame = np.zeros((H, W), np.uint8)
    synth.disc_frame(H, W, c, tw, darker, out=frame)
    ij = np.array([c, (c[0] + 3, c[1]), (c[0], c[1] - 3), (c[0] - 2, c[1] + 2)], np.int32)
    return Case(f"disc tw {tw} {'dark' if darker else 'bright'}", frame[None], ij, np.zeros(len(ij), np.int32), 0, 128, darker, 8,
                float(tw), [(c[0], c[1], None, None, None)] * len(ij))


MOVE_DEG, MOVE_STEP, MOVE_N, STOP_N = 30, 3.0, 8, 4


def _moving_case():
    """The (12, 5) ellipse at MOVE_DEG: MOVE_N steps forwards along its long axis, STOP_N steps at rest, MOVE_N steps back."""
    phi = math.radians(MOVE_DEG)
    along = [MOVE_STEP * k for k in range(MOVE_N + 1)] + [MOVE_STEP * MOVE_N] * STOP_N + [MOVE_STEP * (MOVE_N - 1 - k) for k in range(MOVE_N)]
    frames, ij = [], []
    for k, s in enumerate(along):
        cy, cx = 50.0 + s * math.sin(phi), 60.0 + s * math.cos(phi)
        frames.append(ellipse_frame(cy, cx, 12, 5, MOVE_DEG, 40, [7, k]))
        ij.append((int(round(cy)) + 1, int(round(cx)) + 1))
    n = len(ij)
    return Case("moving ellipse", np.stack(frames), np.array(ij, np.int32), np.arange(n, dtype=np.int32), 25, 128, True, 8, 25.0, [None] * n)


def _degenerate_cases():
    out = []
    flat = np.full((1, H, W), 128, np.uint8)
    ij = np.array([(60, 80), (1, 1), (H, W)], np.int32)
    out.append(Case("flat", flat, ij, np.zeros(3, np.int32), 25, 128, True, 8, 25.0, [None] * 3))
    noisy = np.clip(floor_frame(3), 0, 255).astype(np.uint8)[None]
    for mc in (8, 1):            # the floor's own noise: nothing at 8, a few pixels at 1
        out.append(Case(f"empty floor min_contrast {mc}", noisy, np.array([(60, 80), (30, 20)], np.int32), np.zeros(2, np.int32),
                        12, 128, True, mc, 12.0, [None] * 2))
    for darker, fill in ((True, 255), (False, 0), (True, 0)):
        frame = np.zeros((H, W), np.uint8)
        synth.disc_frame(H, W, (2, 3), 10, darker, out=frame)
        out.append(Case(f"corner disc {'dark' if darker else 'bright'} fill {fill}", frame[None],
                        np.array([(2, 3), (1, 1), (-5, -7), (4, 2)], np.int32), np.zeros(4, np.int32), 10, fill, darker, 8, 10.0, [None] * 4))
    # a disc of value 60 and, 14 px to its right, a smaller one of value 0: inside the patch of R = 25 and above half the
    # target's contrast, so the rule counts it (the known limit); at R = 10 it lies outside
    two = np.full((H, W), 128, np.uint8)
    yy, xx = np.ogrid[0:H, 0:W]
    two[(yy - 59) ** 2 + (xx - 79) ** 2 <= 36] = 60
    two[(yy - 59) ** 2 + (xx - 93) ** 2 <= 9] = 0
    for R in (25, 10):
        out.append(Case(f"second object R {R}", two[None], np.array([(60, 80)], np.int32), np.zeros(1, np.int32), R, 128, True, 8, 25.0, [None]))
    return out


_CASES = None
_REF = {}


def cases():
    global _CASES
    if _CASES is None:
        c = [_ellipse_case(12, 5, 25, 40), _ellipse_case(12, 5, 25, 220), _ellipse_case(6, 3, 12, 40), _ellipse_case(6, 3, 12, 220)]
        c += [_disc_case(tw, d) for tw in (10, 25) for d in (True, False)]
        c.append(_moving_case())
        c += _degenerate_cases()
        _CASES = c
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def reference(c):
    """(shape [n, 6] float64, sums [n, 8] int32) of the restatement for a case, computed once and read-only."""
    if c.name not in _REF:
        R = c.radius or SR.default_radius(c.tw)
        shp, words = SR.shapes(c.frames, c.ij, c.fi, R, c.fill, c.darker, c.min_contrast)
        shp.setflags(write=False)
        words.setflags(write=False)
        _REF[c.name] = (shp, words)
    return _REF[c.name]


def angle_error_deg(theta, deg):
    """|theta - deg| modulo 180 degrees."""
    e = (math.degrees(theta) - deg) % 180.0
    return min(e, 180.0 - e)
