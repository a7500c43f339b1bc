"""The two scenes tests/test_exclusive_cpu.py and tests/test_gpu_exclusive.py share: 41 frames of 100 x 140, background 128,
target width 10 (l = 29), two dark discs of radius 5 that move 2 pixels per frame towards and past each other.
    "through"  window 21, both discs of value 0 in ONE row: they pass through each other (and overlap for a few frames)
    "passing"  window 41, values 0 and 60 twelve rows apart: the weak target's window sees the strong blob as it passes
Independent chains end on one disc in both.  Also the walks the tests compare: independent chains and the exclusive walk over
the oracle's Float64 maps (tests/peaks_restatement.py for the picks, tests/exclusive_restatement.py for the step), and the
error of a walk against the nearer labelling.  TEST HELPER: nothing here loads the library under test."""
import math

import numpy as np

import exclusive_restatement as er
import peaks_restatement as pr

H, W, TW, L, BKGD, NF = 100, 140, 10, 29, 128, 41
MIN_DISTANCE, RATIO, K = 10, 0.5, 4

SCENES = {
    # name: (window, disc values, centres at frame k)
    "through": (21, (0, 0), lambda k: [(50, 30 + 2 * k), (50, 110 - 2 * k)]),
    "passing": (41, (0, 60), lambda k: [(44, 30 + 2 * k), (56, 110 - 2 * k)]),
}
# steps (of 40) whose error against the nearer labelling exceeds 3 px in the Float64 walk: the yardstick for the GPU's cap
FLOAT64_STEPS_ABOVE_3PX = {"through": 5, "passing": 4}
GPU_STEPS_ABOVE_3PX = 8       # the margin is for FP32 tie-breaks among mirror-equal responses; a collapse costs 20 or more


def draw(hw, discs, radius=TW // 2, bkgd=BKGD):
    """A frame with dark discs: [(centre (row, col) 1-based, value)]."""
    f = np.full(hw, bkgd, np.uint8)
    yy, xx = np.ogrid[0:hw[0], 0:hw[1]]
    for (ci, cj), v in discs:
        f[(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= radius * radius] = v
    return f


class Scene:
    def __init__(self, name):
        ws, values, centres = SCENES[name]
        self.name, self.hw, self.tw, self.fill = name, (H, W), TW, BKGD
        self.ws, self.radii, self.values = (ws, ws), (ws // 2, ws // 2), values
        self.truth = [centres(k) for k in range(NF)]
        self.frames = np.stack([draw(self.hw, list(zip(self.truth[k], values))) for k in range(NF)])
        self.starts = self.truth[0]


_CACHE = {}


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = Scene(name)
    return _CACHE[name]


def errors(track, truth):
    """Per step the error against the nearer labelling: the smaller, over the two ways to match two targets to two discs, of the
    larger distance.  track[k] and truth[k]: two (row, col) each."""
    d = lambda p, q: math.hypot(p[0] - q[0], p[1] - q[1])
    return [min(max(d(a, ta), d(b, tb)), max(d(a, tb), d(b, ta))) for (a, b), (ta, tb) in zip(track, truth)]


def steps_above(track, truth, px=3):
    return sum(e > px for e in errors(track, truth)[1:])


def min_assigned_distance2(track, states):
    """The least squared distance between two targets assigned (state >= 1) in the same step; None if no step has two."""
    best = None
    for pos, st in zip(track[1:], states):
        for a in range(len(pos)):
            for b in range(a + 1, len(pos)):
                if st[a] >= 1 and st[b] >= 1:
                    d2 = (int(pos[a][0]) - int(pos[b][0])) ** 2 + (int(pos[a][1]) - int(pos[b][1])) ** 2
                    best = d2 if best is None else min(best, d2)
    return best


def walk_float64(oracle, sc):
    """(independent chains, exclusive walk, its states) over the oracle's Float64 maps, every chain started on its disc at frame 0
    (filed as given) and walked over frames 1 ... 40.  Tracks: [frame][target] = (row, col); states: [step - 1][target]."""
    Kn = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    ind, exc, states = [list(sc.starts)], [list(sc.starts)], []
    for k in range(1, NF):
        ind.append([tuple(int(v) for v in oracle.detect(sc.frames[k], sc.fill, Kn, sc.radii, g)) for g in ind[-1]])
        lists = []
        for g in exc[-1]:
            pos, R = oracle.detect(sc.frames[k], sc.fill, Kn, sc.radii, g, want_resp=True)
            lists.append(pr.select(R, g, sc.radii, sc.hw, pos, K, MIN_DISTANCE))
        out, st = er.assign(np.array(exc[-1]), np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]),
                            np.array([l[2] for l in lists]), MIN_DISTANCE, RATIO)
        exc.append([tuple(int(v) for v in p) for p in out])
        states.append([int(s) for s in st])
    return ind, exc, states
