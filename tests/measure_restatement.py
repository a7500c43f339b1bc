"""NumPy restatement of what pdog_measure / pdog_subpixel compute, and the clip the accuracy condition is stated on.
The library is tested bit for bit against this file.

Two parts of different standing:
  * the five RESPONSES of a position are the reference's buff[I] (src/PawsomeTracker.jl:57) at the position and its four
    neighbours; they come from the C oracle (oracle/dog_oracle.c: dense l x l Float64, kernel column-major order, product
    and sum rounded apart, PaddedView fill) through a 3 x 3 window centred on the position;
  * the SUB-PIXEL RULE is this library's addition, not the reference's: per axis a parabola through three values.

Float64 throughout, each operation rounded on its own (NumPy never fuses).  Test code only: the library never imports it."""
import numpy as np


def clamp_ij(h, w, ij):
    """A position outside the frame is clamped into it first (the tracker's own outputs are, :61)."""
    return min(max(int(ij[0]), 1), int(h)), min(max(int(ij[1]), 1), int(w))


def offset(c, m, p):
    """One axis: c the value at the position, m at the lower-index neighbour, p at the higher one.  0 unless the position
    is a strict maximum along the axis in the sense den < 0 (flat patches and NaN give 0), else the parabola's vertex
    (0.5 num) / den clamped to half a pixel."""
    c, m, p = np.float64(c), np.float64(m), np.float64(p)
    with np.errstate(all="ignore"):
        den = (m - c) + (p - c)
        num = m - p
        if not den < 0:
            return np.float64(0.0)
        off = (np.float64(0.5) * num) / den
    if off > 0.5:
        off = np.float64(0.5)
    if off < -0.5:
        off = np.float64(-0.5)
    return off


def subpixel(r5, ij):
    """r5 = {c, up, down, left, right} at the 1-based (row, col) position ij -> (row, col) in Float64."""
    c, up, down, left, right = (np.float64(v) for v in r5)
    return (np.float64(int(ij[0])) + offset(c, up, down), np.float64(int(ij[1])) + offset(c, left, right))


def resp5(oracle, frame, fill, K, ij):
    """The reference's response at ij (clamped into the frame) and at its four neighbours, {c, up, down, left, right}."""
    i, j = clamp_ij(frame.shape[0], frame.shape[1], ij)
    _, r = oracle.detect(frame, fill, K, (1, 1), (i, j), want_resp=True)
    return np.array([r[1, 1], r[0, 1], r[2, 1], r[1, 0], r[1, 2]], np.float64)


def measure(oracle, frames, fill, K, ijs, frame_index=None):
    """n positions: (sub [n, 2], resp5 [n, 5]) as pdog_measure writes them."""
    n = len(ijs)
    sub, r5 = np.empty((n, 2), np.float64), np.empty((n, 5), np.float64)
    for b in range(n):
        f = frames[b if frame_index is None else int(frame_index[b])]
        r5[b] = resp5(oracle, f, fill, K, ijs[b])
        sub[b] = subpixel(r5[b], clamp_ij(f.shape[0], f.shape[1], ijs[b]))
    return sub, r5


# ---- the clip of the accuracy condition: a seeded version of the reference's own test recipe ----
# test/test-basic-test.jl: 100 x 100 frames, 10 s at 24 fps (241 frames), a disc of width 10 on an Archimedean spiral of
# 5 loops that starts at (50, 50) and reaches 0.8 * 50 px, equal steps in arc length.  The reference rounds the centres to
# whole pixels; here they stay real numbers — spiral + N(0, JITTER) per axis — and the disc is drawn by area coverage
# (SS x SS samples per pixel), so that "the true centre" means something below a pixel.  +-NOISE grey levels, uniform.
H = W = 100
NFRAMES = 241
DISC_WIDTH = 10
LOOPS = 5
JITTER = 0.3
NOISE = 2
SS = 8


def spiral_centres(seed, nframes=NFRAMES, start=(50.0, 50.0), reach=40.0):
    """[nframes, 2] Float64 1-based (row, col) centres."""
    a = reach / LOOPS / (2 * np.pi)
    th = np.linspace(0.0, LOOPS * 2 * np.pi, 200001)
    arc = a / 2 * (th * np.sqrt(1 + th * th) + np.arcsinh(th))          # len(theta, a) of the reference's helper
    theta = np.interp(np.linspace(0.0, arc[-1], nframes + 1)[1:], arc, th)
    rng = np.random.Generator(np.random.PCG64(seed))
    p = np.stack([a * theta * np.cos(theta), a * theta * np.sin(theta)], 1) + rng.normal(0.0, JITTER, (nframes, 2))
    return p - p[0] + np.asarray(start, np.float64)


def disc_frame(centre, darker, rng, h=H, w=W):
    """One frame: background 128, the disc 0 (dark) or 255 (bright) by area coverage, then the noise."""
    s = (np.arange(SS) + 0.5) / SS - 0.5
    yy = (np.arange(1, h + 1)[:, None] + s[None, :]).reshape(-1)          # sample rows, SS per pixel row
    xx = (np.arange(1, w + 1)[:, None] + s[None, :]).reshape(-1)
    inside = (yy[:, None] - centre[0]) ** 2 + (xx[None, :] - centre[1]) ** 2 <= (DISC_WIDTH / 2) ** 2
    cover = inside.reshape(h, SS, w, SS).mean((1, 3))
    target = 0.0 if darker else 255.0
    img = np.rint(128.0 + (target - 128.0) * cover)
    img += rng.integers(-NOISE, NOISE + 1, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def spiral_clip(seed, darker, upto=NFRAMES):
    """(frames uint8 [upto, H, W], centres Float64 [upto, 2]): the first `upto` frames of the NFRAMES-frame clip."""
    centres = spiral_centres(seed)[:upto]
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    return np.stack([disc_frame(c, darker, rng) for c in centres]), centres


def oracle_chain(oracle, frames, target_width, window_size, darker, start=(50, 50)):
    """The reference's frame loop (src/PawsomeTracker.jl:159-169) on the oracle: (positions, fill, K)."""
    from oracle.dog_oracle import OracleTracker
    ot = OracleTracker(frames[0], target_width, window_size, darker, oracle)
    ijs = [ot(start)]
    for f in frames[1:]:
        ot.data[...] = f
        ijs.append(ot(ijs[-1]))
    return ijs, ot.fill, ot.kernel


def rmse(est, truth):
    d = np.asarray(est, np.float64) - np.asarray(truth, np.float64)
    return float(np.sqrt((d * d).sum(1).mean()))
