"""The scenes tests/test_peaks_cpu.py and tests/test_gpu_peaks.py share: a 120 x 160 frame, background 128, target width 10
(l = 29), dark discs of radius 5 whose centres lie at least 25 pixels apart, and ONE window that covers them all.  The
four-disc scenes hold the values 0 / 30 / 60 / 90: by contrast the DoG responses at the centres differ by a quarter of the
strongest one, against ~1e-6 between the Float64 oracle and any kernel family's float32 order, so both arithmetics rank them
alike (test_peaks_cpu.py asserts it).  TEST HELPER: nothing here loads the library under test."""
import numpy as np

H, W, TW, L, BKGD = 120, 160, 10, 29, 128

# name -> [(centre (row, col) 1-based, value)], listed in contrast order: the expected pick order
SCENES = {
    "spread":  [((30, 40), 0), ((80, 120), 30), ((35, 110), 60), ((85, 45), 90)],
    "against the scan": [((70, 130), 0), ((40, 30), 30), ((90, 60), 60), ((30, 90), 90)],    # contrast order runs against idx order
    "a tight square": [((40, 60), 0), ((40, 85), 30), ((65, 60), 60), ((65, 85), 90)],       # neighbours exactly 25 apart
}
# two identical discs: exactly equal responses; the column-major first — the larger row here — comes first
TWINS = [((70, 50), 0), ((40, 110), 0)]


class Scene:
    def __init__(self, discs, ws=(101, 141), guess=(60, 80)):
        self.hw, self.tw, self.l, self.fill = (H, W), TW, L, BKGD
        self.ws, self.radii, self.guess = ws, (ws[0] // 2, ws[1] // 2), guess
        self.centres = [c for c, _ in discs]
        self.values = [v for _, v in discs]
        f = np.full((H, W), BKGD, np.uint8)
        yy, xx = np.ogrid[0:H, 0:W]
        for (ci, cj), v in discs:
            f[(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= (TW // 2) ** 2] = v
        self.frame = f


_CACHE = {}


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = Scene(TWINS if name == "twins" else SCENES[name])
    return _CACHE[name]
