"""The scenes tests/test_motion_cpu.py and tests/test_gpu_motion.py share: the two of tests/exclusive_scenes.py, unchanged, and
two with ONE dark disc of radius 5 (value 0, background 128, target width 10) on 17 frames of 100 x 140 that moves 7 pixels
per frame along row 50, tracked with an 11 x 11 window and k = 1:
    "fast"    the disc centred at (50, 15 + 7 f) on frame f: a plain chain needs a 15 x 15 window to follow it
    "vanish"  the same, with frames 9 ... 16 flat at 128: coast 3, min_response 1e-3
Also the walks the tests compare — the motion walk over the oracle's Float64 maps (tests/peaks_restatement.py for the picks,
tests/motion_restatement.py for the step) and the oracle's plain chain — and the error of a walk against the TRUE labelling
(target t on disc t).  TEST HELPER: nothing here loads the library under test."""
import math

import numpy as np

import exclusive_scenes as es
import motion_restatement as mr
import peaks_restatement as pr

H, W, TW, BKGD = es.H, es.W, es.TW, es.BKGD
FAST_NF, FAST_WS, FAST_SPEED = 17, 11, 7
COAST, MIN_RESPONSE = 8, 0.0            # the Python layer's defaults: what "through" and "passing" walk with
VANISH_FROM, VANISH_COAST, VANISH_MIN_RESPONSE = 9, 3, 1e-3
# "vanish": held from step 9 on; three steps along v = (0, 7), then at rest
VANISH_TAIL = [(50, 78), (50, 85), (50, 92)] + [(50, 92)] * 5

NAMES = ("through", "passing", "fast", "vanish")


class Scene:
    """What es.Scene carries, plus the step's parameters."""

    def __init__(self, name):
        self.name, self.hw, self.tw, self.fill = name, (H, W), TW, BKGD
        if name in es.SCENES:
            base = es.scene(name)
            self.ws, self.radii, self.frames, self.truth = base.ws, base.radii, base.frames, base.truth
            self.k, self.min_distance, self.ratio, self.min_response, self.coast = es.K, es.MIN_DISTANCE, es.RATIO, MIN_RESPONSE, COAST
        else:
            self.ws, self.radii = (FAST_WS, FAST_WS), (FAST_WS // 2, FAST_WS // 2)
            self.truth = [[(50, 15 + FAST_SPEED * f)] for f in range(FAST_NF)]
            self.frames = np.stack([es.draw(self.hw, [(c[0], 0)]) for c in self.truth])
            self.k, self.min_distance, self.ratio, self.min_response, self.coast = 1, es.MIN_DISTANCE, es.RATIO, MIN_RESPONSE, COAST
            if name == "vanish":
                self.frames[VANISH_FROM:] = BKGD
                self.min_response, self.coast = VANISH_MIN_RESPONSE, VANISH_COAST
                self.truth = self.truth[:VANISH_FROM] + [[p] for p in VANISH_TAIL]
        self.nf = len(self.frames)
        self.starts = self.truth[0]


_CACHE = {}


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = Scene(name)
    return _CACHE[name]


def errors_true(track, truth):
    """Per step the error against the TRUE labelling: the largest distance of a target from its own disc."""
    return [max(math.hypot(p[0] - q[0], p[1] - q[1]) for p, q in zip(pos, tru)) for pos, tru in zip(track, truth)]


def steps_above_true(track, truth, px=3):
    return sum(e > px for e in errors_true(track, truth)[1:])


def walk_float64(oracle, sc, min_response=None, frames=None):
    """(track, states, responses, contested) of the motion walk over the oracle's Float64 maps, every target started on its
    disc at frame 0 (filed as given), at rest, and walked over frames 1 ... nf - 1.  track[frame][target] = (row, col);
    states, responses (pick 1's value) and contested [step - 1][target]."""
    Kn = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    frames = sc.frames if frames is None else frames
    m = sc.min_response if min_response is None else min_response
    T = len(sc.starts)
    pos, ms = np.array(sc.starts, np.int32), np.zeros((T, 4), np.int32)
    nxt = np.array([(mr.clamp(p[0], H), mr.clamp(p[1], W)) for p in pos], np.int32)
    track, states, resp, cont = [list(sc.starts)], [], [], []
    for f in range(1, sc.nf):
        lists = []
        for g in nxt:
            p1, R = oracle.detect(frames[f], sc.fill, Kn, sc.radii, g, want_resp=True)
            lists.append(pr.select(R, g, sc.radii, sc.hw, p1, sc.k, sc.min_distance))
        pos, st, nxt2, ms, c = mr.step(pos, ms, np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]),
                                       np.array([l[2] for l in lists]), sc.hw, sc.min_distance, sc.ratio, m, sc.coast, detail=True)
        # the guess the walk hands on IS the prediction the next step forms
        assert all(tuple(nxt2[t]) == (mr.clamp(int(pos[t, 0]) + int(ms[t, 0]), H), mr.clamp(int(pos[t, 1]) + int(ms[t, 1]), W)) for t in range(T))
        nxt = nxt2
        track.append([tuple(int(v) for v in p) for p in pos])
        states.append([int(s) for s in st])
        resp.append([float(l[1][0]) for l in lists])
        cont.append([bool(v) for v in c])
    return track, states, resp, cont


def plain_chain_float64(oracle, sc):
    """The oracle's plain chain (the reference's functor, step after step) for the scene's first target."""
    Kn = oracle.dog_kernel(oracle.sigma(sc.tw), True)
    track = [[sc.starts[0]]]
    for f in range(1, sc.nf):
        track.append([tuple(int(v) for v in oracle.detect(sc.frames[f], sc.fill, Kn, sc.radii, track[-1][0]))])
    return track
