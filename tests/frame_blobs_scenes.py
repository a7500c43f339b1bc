"""The scenes of the frame-blob tests (include/pawsome_frame_blobs.h): masks that are hard for a tiled labelling — tiles are
64 x 64 pixels — drawn at any frame size, and the bootstrap video of track_video(find="frame").  TEST HELPER: nothing here
loads the library under test.

A scene is a bool pattern [h, w].  `frames(h, w, darker)` draws every scene as one frame of a stack: the floor around level
128 with a texture that stays below the least contrast 8, the pattern's pixels at contrasts 8 ... 68 (so that Ss is no multiple
of n); the `darker=False` stack is 255 minus the other one and is read against level 127, which gives every pixel the same
contrast and every blob the same words."""
import numpy as np

TILE = 64
LEVEL = {True: 128, False: 127}
HEIGHTS, WIDTHS = (1, 2, 31, 33, 70), (1, 63, 64, 65, 127, 129, 200)


def _empty(h, w):
    return np.zeros((h, w), bool)


def _full(h, w):
    return np.ones((h, w), bool)


def _corners(h, w):
    m = _empty(h, w)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = True
    return m


def _spiral(h, w):
    """A one-pixel-wide spiral from the top-left corner inwards, turns two pixels apart: one blob at either connectivity whose
    pixels lie as far apart, along the blob, as pixels of an h x w frame can."""
    m = _empty(h, w)
    k = 0
    while 2 * k <= h - 1 - 2 * k and 2 * k <= w - 1 - 2 * k:
        t, b, l, r = 2 * k, h - 1 - 2 * k, 2 * k, w - 1 - 2 * k
        m[t, max(l - 2, 0):r + 1] = True        # the top side starts where the previous turn's left side ended
        m[t:b + 1, r] = True
        m[b, l:r + 1] = True
        m[min(t + 2, b):b + 1, l] = True        # the left side stops two rows short: the next turn's top side goes on from there
        k += 1
    return m


def _comb(h, w):
    """Teeth in every other column that join only in the LAST row: every equivalence is found at the very end of a raster scan."""
    m = _empty(h, w)
    m[:, ::2] = True
    m[h - 1, :] = True
    return m


def _checkerboard(h, w):
    rr, cc = np.ogrid[0:h, 0:w]
    return (rr + cc) % 2 == 0


def _staircases(h, w):
    """Two diagonals, one pixel per row: r == c runs through the tile corners (63, 63) -> (64, 64), r + c == 127 through
    (63, 64) -> (64, 63), and a third one column off.  One blob each at connectivity 8, single pixels at 4."""
    rr, cc = np.ogrid[0:h, 0:w]
    return (rr == cc) | (rr + cc == 2 * TILE - 1) | (rr + 5 == cc - 2 * TILE)


def _lattice(h, w):
    """One blob that crosses every tile border: a row and a column through the middle of every tile."""
    rr, cc = np.ogrid[0:h, 0:w]
    return (rr % TILE == TILE // 2) | (cc % TILE == TILE // 2) | ((rr == 0) & (cc >= 0))


def _neighbours(h, w):
    """Pairs of blobs ONE PIXEL APART with a tile border between them — bars in columns 62 | 64 and 63 | 65 and in rows
    62 | 64 — and never joined, at either connectivity."""
    m = _empty(h, w)
    m[0:h // 2, TILE - 2:TILE - 1] = True
    m[0:h // 2, TILE:TILE + 1] = True
    m[h // 2 + 1:, TILE - 1:TILE] = True
    m[h // 2 + 1:, TILE + 1:TILE + 2] = True
    m[TILE - 2:TILE - 1, 2 * TILE + 4:] = True
    m[TILE:TILE + 1, 2 * TILE + 4:] = True
    return m


def _noise(density, seed):
    def make(h, w):
        return np.random.default_rng([seed, h, w]).random((h, w)) < density
    return make


SCENES = {
    "empty": _empty, "full": _full, "corners": _corners, "spiral": _spiral, "comb": _comb, "checkerboard": _checkerboard,
    "staircases": _staircases, "lattice": _lattice, "neighbours": _neighbours,
    "noise 0.41": _noise(0.41, 41), "noise 0.59": _noise(0.59, 59),       # either side of the percolation thresholds
}
NAMES = tuple(SCENES)


def pattern(name, h, w):
    return SCENES[name](h, w)


# The shapes beyond the tile's neighbourhood, each the smallest that reaches a path of the kernels, with the scenes it runs:
#   (520, 520)      1057 blocks of 256 pixels: the scan of the blocks' counts (1024 at a time) has a second pass; 9 x 9 tiles,
#                   a width that is a multiple of 4; the checkerboard has 135 200 blobs at connectivity 4
#   (1037, 1041)    4217 blocks: five passes; 17 x 17 tiles, both sides odd
#   (3, 2^21)       the widest size admitted: 32 768 tile columns, single addends of 2^48, a full frame's Sxx at 0.9999993 of 2^63
#   (9000, 64)      141 tile rows and ONE tile column: no vertical border
#   (3 024 617, 1)  the tallest size admitted: 47 260 tile rows, a full frame's Syy at 0.99999993 of 2^63
LARGE = (
    ((520, 520), NAMES),
    ((1037, 1041), ("full", "spiral", "comb", "checkerboard", "lattice", "staircases", "noise 0.41", "noise 0.59")),
    ((3, 1 << 21), ("full", "comb", "noise 0.59")),
    ((9000, 64), ("full", "spiral", "lattice", "noise 0.59")),
    ((3024617, 1), ("full", "checkerboard", "noise 0.59")),
)


def draw(mask, darker=True, seed=0):
    """The frame of a pattern: uint8 [h, w]."""
    h, w = mask.shape
    rng = np.random.default_rng([seed, h, w, int(mask.sum())])
    s = np.where(mask, rng.integers(8, 69, (h, w)), rng.integers(-5, 8, (h, w)))          # the contrast of every pixel
    f = (128 - s).astype(np.uint8)
    return f if darker else (255 - f).astype(np.uint8)


def noise_frames(density, n, h, w, darker=True):
    """n frames of noise at h x w, every one with a mask and contrasts of its own: uint8 [n, h, w]."""
    return np.stack([draw(_noise(density, 1000 + k)(h, w), darker, k) for k in range(n)])


def frames(h, w, darker=True):
    """Every scene at h x w, one frame each, in NAMES' order: uint8 [len(NAMES), h, w]."""
    return np.stack([draw(pattern(name, h, w), darker, k) for k, name in enumerate(NAMES)])


# ---- the bootstrap video of track_video(find="frame") ----
BOOT_H, BOOT_W, BOOT_NF, BOOT_TW = 120, 160, 21, 11
BOOT_RADII = (6, 5, 4)                                             # 113, 81 and 49 pixels: target 0 is the largest
BOOT_STARTS = np.array([(20, 25), (100, 30), (30, 135)], float)    # 1-based centres on frame 0: all outside the centre window
BOOT_STEPS = np.array([(0.5, 0.5), (-0.5, 0.5), (0.5, -0.5)])
BOOT_ARGS = dict(rate=24, start=0, stop=BOOT_NF / 24, fps=24, target_width=BOOT_TW)


def boot_centres(k):
    return np.rint(BOOT_STARTS + k * BOOT_STEPS).astype(int)


def boot_video(furniture=False):
    """21 frames of 120 x 160 at level 128 with three dark discs that start near the walls — none inside the reference's
    bootstrap window, 30 x 40 pixels around (60, 80) — and walk half a pixel per frame.  furniture=True adds what never moves: a
    dark slab in the middle of the arena and a stain, both darker than the discs; returns (frames, the empty arena)."""
    arena = np.full((BOOT_H, BOOT_W), 128, np.uint8)
    if furniture:
        arena[50:72, 66:96] = 20
        arena[100:112, 120:150] = 35
    video = np.repeat(arena[None], BOOT_NF, 0)
    yy, xx = np.ogrid[0:BOOT_H, 0:BOOT_W]
    for k in range(BOOT_NF):
        for (ci, cj), rad, v in zip(boot_centres(k), BOOT_RADII, (40, 60, 50)):
            video[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= rad * rad] = v
    return video, arena
