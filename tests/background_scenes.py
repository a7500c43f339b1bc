"""The clutter scene of the background model (include/pawsome_background.h), seeded: an arena whose floor brightens from left to
right under +-2 noise, a STATIC disc of value 0 — a hole — a few rows off the path of a moving disc of value 60 — the animal.
On the raw frames the hole responds more strongly than the animal and lies within half a window of its path: the plain chain
parks on it.  It is part of every frame, so it is part of the median, and the subtracted frames do not show it.

    frame k = min(floor + noise_k, hole, animal_k)       noise_k: one draw of PCG64(7), in frame order
    floor[i, j] = 100 + floor(0.3 * j);  hole: width 10 at (64, 80);  animal k: width 10 at (60, 20 + 2 k)      (0-based)

`scene(darker=False)` is the bright twin, 255 - frame; `scene(second=True)` adds a second animal on row 25 walking the other
way, far from the first and from the hole, for the loops that take a group.  Test data only: nothing here loads the library."""
from types import SimpleNamespace

import numpy as np

H, W, NF, TW, WS = 120, 160, 60, 10, 21
SEED, NOISE = 7, 2
HOLE = (64, 80)            # 0-based centre; its row offset from the path is 4 (the conditions hold for 3 ... 6)
PATH_ROW, COL0, SPEED = 60, 20, 2
ROW2, COL2 = 25, 140       # the second animal: row 25, from column 140 leftwards


def _disc(frame, centre, width, value):
    i, j = np.mgrid[0:H, 0:W]
    r = width / 2.0
    frame[(i - centre[0]) ** 2 + (j - centre[1]) ** 2 <= r * r] = value


def scene(darker=True, second=False, hole_row=HOLE[0]):
    """frames uint8 [NF, H, W]; truth[t][k] the 1-based (row, col) of animal t on frame k; starts = truth[:, 0]."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    floor = (100 + np.floor(0.3 * np.arange(W))).astype(np.int16)[None, :].repeat(H, 0)
    frames = np.empty((NF, H, W), np.uint8)
    paths = [[(PATH_ROW, COL0 + SPEED * k) for k in range(NF)]]
    if second:
        paths.append([(ROW2, COL2 - SPEED * k) for k in range(NF)])
    for k in range(NF):
        f = floor + rng.integers(-NOISE, NOISE + 1, (H, W)).astype(np.int16)      # one draw per frame
        f = np.clip(f, 0, 255).astype(np.uint8)
        _disc(f, (hole_row, HOLE[1]), TW, 0)
        for p in paths:
            animal = np.full((H, W), 255, np.uint8)
            _disc(animal, p[k], TW, 60)
            f = np.minimum(f, animal)
        frames[k] = f
    if not darker:
        frames = 255 - frames
    truth = [[(i + 1, j + 1) for i, j in p] for p in paths]
    return SimpleNamespace(frames=frames, truth=truth, starts=[p[0] for p in truth], darker=darker, nf=NF, tw=TW, ws=WS, hw=(H, W))


def errors(track, truth):
    """Per step the Euclidean distance of a chain's positions to the truth."""
    return [float(np.hypot(a[0] - b[0], a[1] - b[1])) for a, b in zip(track, truth)]
