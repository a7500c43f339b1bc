"""NumPy restatement of the reference's diagnostic overlay (src/diagnose.jl:26-38): what `dia(img, point)` draws
into its 360 x 640 buffer for one frame.  The library's pdog_diag_* path is tested bit for bit against this file.
Nothing here can run Julia, so the restatement rests on recollections of the Julia packages the reference pins
(ImageTransformations 0.10, ImageDraw 0.1/0.2, DataStructures' CircularBuffer); nobody has checked them here:

  (a) Float64(::N0f8) is raw / 255.0 (the DoG path's assumption too).
  (b) imresize! computes its coordinates and weights with a separate multiply and add (no fused multiply-add) and
      combines the four taps with the row index innermost.
  (c) the conversion back to N0f8 is round(v * 255), ties to even.
  (d) ImageDraw's filled ellipse (CirclePointRadius) draws the pixels with ((a-qi)/r)^2 + ((b-qj)/r)^2 < 1, strict.
  (e) ImageDraw's Path draws each segment with the Bresenham variant in `bresenham` below, from the older point to
      the newer one.
(a)-(c) can move a pixel by at most one grey level, and only at an exact tie; (d) and (e) decide which pixels are
drawn.  The label (renderstring!, :35) is not restated: it needs FreeType and the reference's font asset, and the
library does not rasterise text.

Float64 throughout, each product and sum rounded on its own (NumPy and Python never fuse), rounding half to even
(np.rint, Julia's round).  Test code only: the library never imports it."""
import numpy as np

H, W = 360, 640        # DIAGNOSTIC_VIDEO_SIZE, src/diagnose.jl:2
TRACE = 100            # TRACE_BUFFER_SIZE, src/diagnose.jl:3
RADIUS = 2             # CirclePointRadius(ij, 2), :36


def clamp_ij(h, w, ij):
    """A position outside the frame is clamped into it first (the tracker's own outputs are, :61)."""
    return min(max(int(ij[0]), 1), int(h)), min(max(int(ij[1]), 1), int(w))


def point(h, w, ij):
    """:31 with update_ratio! (:26-28): ratio first (360 / h, 640 / w), then the product, then round.
    The result lies in [0, 360] x [0, 640]; 0 is off the buffer (row 1 of a 1080-row frame gives rint(1/3) = 0)."""
    i, j = clamp_ij(h, w, ij)
    r = (H / h, W / w)
    return int(np.rint(i * r[0])), int(np.rint(j * r[1]))


def axis_map(n_in, n_out, clamp):
    """imresize! (bilinear, no antialiasing, centre-aligned) along one axis: 1-based first tap, second tap, weight
    of the second tap for every output index.  A second tap whose weight is 0 is set to the first: 0 * p adds an exact
    +0, so the value is the same and the reader touches one source row (column) less."""
    s = n_in / n_out
    off = 0.5 - s * 0.5
    y = np.arange(1, n_out + 1, dtype=np.float64) * s + off
    if clamp:
        y = np.clip(y, 1.0, float(n_in))
    iy = np.floor(y)
    f = y - iy
    i0 = iy.astype(np.int64)
    assert i0.min() >= 1 and i0.max() <= n_in
    i1 = np.where(f == 0.0, i0, np.minimum(i0 + 1, n_in))
    return i0, i1, f


def maps(h, w):
    clamp = h < H or w < W           # either axis upsamples: both coordinates are clamped into the frame
    return axis_map(h, H, clamp), axis_map(w, W, clamp)


def resize(img):
    """imresize!(buffer, img) of one h x w uint8 frame -> 360 x 640 uint8."""
    img = np.asarray(img)
    h, w = img.shape
    (i0, i1, fy), (j0, j1, fx) = maps(h, w)
    p = img.astype(np.float64) / 255.0
    fy, fx = fy[:, None], fx[None, :]
    r0, r1, c0, c1 = (i0 - 1)[:, None], (i1 - 1)[:, None], (j0 - 1)[None, :], (j1 - 1)[None, :]
    v = (1 - fx) * ((1 - fy) * p[r0, c0] + fy * p[r1, c0]) + fx * ((1 - fy) * p[r0, c1] + fy * p[r1, c1])
    return np.clip(np.rint(v * 255), 0, 255).astype(np.uint8)


def _plot(buf, a, b, color):
    if 1 <= a <= H and 1 <= b <= W:          # drawifinbounds!
        buf[a - 1, b - 1] = color


def dot(buf, q, color):
    """draw!(buffer, CirclePointRadius(q, 2), color): ((a-qi)/2)^2 + ((b-qj)/2)^2 < 1, i.e. the 3 x 3 block."""
    for a in range(q[0] - RADIUS, q[0] + RADIUS + 1):
        for b in range(q[1] - RADIUS, q[1] + RADIUS + 1):
            if ((a - q[0]) / RADIUS) ** 2 + ((b - q[1]) / RADIUS) ** 2 < 1:
                _plot(buf, a, b, color)


def segment_pixels(p0, p1):
    """One segment of Path(trace): the (row, col) pixels ImageDraw's bresenham plots inside the buffer, in walk order,
    x = column, y = row, walked from p0 (older) to p1 (newer).  The reference's err = (dx > dy ? dx : -dy) / 2 is a
    Float64 half-integer; it is held doubled here (err2 = 2 err), which is exact."""
    y0, x0 = p0
    y1, x1 = p1
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err2 = dx if dx > dy else -dy
    out = []
    while True:
        if 1 <= y0 <= H and 1 <= x0 <= W:          # drawifinbounds!
            out.append((y0, x0))
        if x0 == x1 and y0 == y1:
            break
        e2 = err2
        if e2 > -2 * dx:
            err2 -= 2 * dy
            x0 += sx
        if e2 < 2 * dy:
            err2 += 2 * dx
            y0 += sy
    return out


def bresenham(buf, p0, p1, color):
    for a, b in segment_pixels(p0, p1):
        buf[a - 1, b - 1] = color


class Diagnose:
    """The reference's `Diagnose` (:5-23) minus label and writer: one trace (a CircularBuffer of TRACE scaled points,
    oldest first) that runs on across calls and frame sizes, as across the files of track(files; ...) (:201-207)."""

    def __init__(self, darker_target=True):
        self.color = 255 if darker_target else 0          # :17
        self.trace = []

    def __call__(self, img, ij):
        """dia(img, point), :30-38: push the scaled point, resize, draw dot and path.  Returns the buffer."""
        img = np.asarray(img)
        h, w = img.shape
        q = point(h, w, ij)
        self.trace.append(q)
        del self.trace[:-TRACE]
        buf = resize(img)
        dot(buf, q, self.color)
        for a, b in zip(self.trace[:-1], self.trace[1:]):
            bresenham(buf, a, b, self.color)
        return buf

    def render(self, frames, ijs):
        return np.stack([self(f, ij) for f, ij in zip(frames, ijs)]) if len(frames) else np.zeros((0, H, W), np.uint8)
