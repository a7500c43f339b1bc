"""Frame stacks behind another memory layout, and the scenes the layout tests run on.

include/pawsome_dog.h: "frame k at d_frames + k*frame_stride, rows row_stride bytes apart" — any row_stride >= w, any
frame_stride >= 0, any base address.  The same pixels behind another layout must give the same response bits and the
same positions ("bit-identical whatever the alignment").  This file builds such layouts on the host
(`make`, `overlapping`, `aliased`) and on the device (`to_device`), the ways a kernel could MISREAD them (`misreadings`:
what the oracle sees if the pitch, the frame stride, the base or the frame's borders are taken wrongly), and the scenes
(`scene`) that tests/test_layout_cpu.py shows to catch every misreading and tests/test_gpu_layout.py hands to the kernels.
Bytes that belong to no frame hold the POISON: the target's own colour, so that slack read as pixels attracts the peak
instead of hiding.  TEST HELPER: nothing here loads the library under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402

TAIL = 64          # poisoned bytes behind the last row, at least


def poison_for(darker):
    return 5 if darker else 250


class Layout:
    """A flat host buffer and where its frames lie: frame k's pixel (i, j) is flat[base + k*frame_stride + i*row_stride + j]."""

    def __init__(self, flat, base, nf, h, w, row_stride, frame_stride):
        self.flat, self.base, self.nf, self.h, self.w = flat, int(base), int(nf), int(h), int(w)
        self.row_stride, self.frame_stride = int(row_stride), int(frame_stride)
        last = self.base + (self.nf - 1) * self.frame_stride + (self.h - 1) * self.row_stride + self.w
        assert self.base >= 0 and self.row_stride >= self.w and self.frame_stride >= 0 and last + TAIL <= flat.size, (base, last, flat.size)

    def _view(self, base, row_stride, frame_stride):
        return np.lib.stride_tricks.as_strided(self.flat[base:], (self.nf, self.h, self.w), (frame_stride, row_stride, 1), writeable=False)

    @property
    def view(self):
        return self._view(self.base, self.row_stride, self.frame_stride)

    def twin(self):
        return np.ascontiguousarray(self.view)

    def describe(self):
        return f"base {self.base} (mod 16: {self.base % 16}) row_stride {self.row_stride} (w {self.w}) frame_stride {self.frame_stride} (h*row_stride {self.h * self.row_stride})"


def make(frames, slack, base, gap, poison):
    """frames: contiguous uint8 [nf, h, w].  row_stride = w + slack, frame_stride = h*row_stride + gap, the view starts at
    byte `base` of a flat buffer filled with `poison`; the view holds exactly `frames`."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3 and frames.flags.c_contiguous and min(slack, base, gap) >= 0
    nf, h, w = frames.shape
    rs = w + slack
    fs = h * rs + gap
    flat = np.full(base + nf * fs + TAIL, poison, np.uint8)
    lay = Layout(flat, base, nf, h, w, rs, fs)
    np.lib.stride_tricks.as_strided(flat[base:], (nf, h, w), (fs, rs, 1))[:] = frames
    assert np.array_equal(lay.view, frames) and (flat[-TAIL:] == poison).all()
    return lay


def overlapping(tall, nf, h, step, slack, base, poison):
    """Frame k is rows k*step ... k*step + h - 1 of ONE tall image (uint8 [(nf-1)*step + h, w]): frame_stride = step*row_stride."""
    tall = np.asarray(tall)
    assert tall.dtype == np.uint8 and tall.shape[0] == (nf - 1) * step + h and step >= 0
    H, w = tall.shape
    rs = w + slack
    flat = np.full(base + H * rs + TAIL, poison, np.uint8)
    np.lib.stride_tricks.as_strided(flat[base:], (H, w), (rs, 1))[:] = tall
    lay = Layout(flat, base, nf, h, w, rs, step * rs)
    assert all(np.array_equal(lay.view[k], tall[k * step:k * step + h]) for k in range(nf))
    return lay


def aliased(frame, nf, slack, base, poison):
    """nf frames that are all the same memory: frame_stride = 0."""
    return overlapping(frame, nf, frame.shape[0], 0, slack, base, poison)


def to_device(lay, clips=None):
    """The same view on the device: the flat buffer uploaded once, then torch.as_strided.  clips = nc: a 4-d view
    [nc, nf/nc, h, w] whose clips are stacked contiguously (stride(0) = (nf/nc)*stride(1)), as detect_chains takes it.
    Asserts the strides and the base alignment that were asked for."""
    import torch
    d_flat = torch.from_numpy(lay.flat).cuda()
    if clips is None:
        v = torch.as_strided(d_flat, (lay.nf, lay.h, lay.w), (lay.frame_stride, lay.row_stride, 1), lay.base)
        assert v.stride(0) == lay.frame_stride and v.stride(1) == lay.row_stride
    else:
        per = lay.nf // clips
        assert per * clips == lay.nf
        v = torch.as_strided(d_flat, (clips, per, lay.h, lay.w), (per * lay.frame_stride, lay.frame_stride, lay.row_stride, 1), lay.base)
        assert v.stride(0) == per * v.stride(1) and v.stride(1) == lay.frame_stride and v.stride(2) == lay.row_stride
    assert v.stride(-1) == 1 and (v.data_ptr() - d_flat.data_ptr()) == lay.base and d_flat.data_ptr() % 16 == 0
    assert v.data_ptr() % 16 == lay.base % 16
    return v


def host_tensor(lay):
    """The view as a HOST tensor of the same strides (what _args.device_frames judges before it looks at the device)."""
    import torch
    return torch.as_strided(torch.from_numpy(lay.flat), (lay.nf, lay.h, lay.w), (lay.frame_stride, lay.row_stride, 1), lay.base)


# ---- the misreadings ----
MISREADINGS = ("pitch = w", "frame_stride = h*row_stride", "base dropped", "slack and gap for fill")


def misreadings(lay, fill):
    """What a kernel that takes the layout wrongly would see, as frames the oracle can be asked about.  The first three are
    views of the same flat buffer [nf, h, w]; the fourth reads on where the fill belongs: right of column w the row's slack
    (and the next row), below row h the gap (and the next frame) — frames [nf, h + pad, w + pad], the frame's own h x w in
    the top-left corner, `fill` where the address leaves the buffer.  Returns {name: frames}."""
    out = {
        MISREADINGS[0]: lay._view(lay.base, lay.w, lay.frame_stride),
        MISREADINGS[1]: lay._view(lay.base, lay.row_stride, lay.h * lay.row_stride),
        MISREADINGS[2]: lay._view(0, lay.row_stride, lay.frame_stride),
    }
    pad_h, pad_w = lay.h, lay.w
    k, i, j = np.ogrid[0:lay.nf, 0:lay.h + pad_h, 0:lay.w + pad_w]
    addr = lay.base + k * lay.frame_stride + i * lay.row_stride + j
    ext = np.where(addr < lay.flat.size, lay.flat[np.minimum(addr, lay.flat.size - 1)], np.uint8(fill)).astype(np.uint8)
    assert np.array_equal(ext[:, :lay.h, :lay.w], lay.view)
    out[MISREADINGS[3]] = ext
    return out


def misread_position(oracle, frames_k, h, w, fill, K, radii, guess):
    """The oracle's position on a misread frame, clamped to the h x w frame as the functor clamps (:61).  For the three
    same-size misreadings the clamp changes nothing."""
    i, j = oracle.detect(frames_k, fill, K, radii, guess)
    return (min(max(i, 1), h), min(max(j, 1), w))


# ---- scenes ----
def tw_for_kernel_len(l):
    for tw10 in range(20, 1400):
        if fr.kernel_len(fr.sigma_of(tw10 / 10)) == l:
            return tw10 / 10
    raise AssertionError(l)


class Scene:
    """nf frames h x w, a target per frame (a disc of the target's colour), and the windows every launch holds: per frame one
    on the disc (inside the frame), one over each of the four borders, one over each of two corners and one with the target
    in its last columns.  `windows` is [(frame, (row, col))] in an order whose frame indices are a non-identity permutation
    with repeats; `position` gives the oracle's answers on the contiguous frames, each computed once."""

    def __init__(self, l, ws, h, w, nf, content, col=None):
        self.l, self.ws, self.h, self.w, self.nf, self.content = l, tuple(ws), h, w, nf, content
        self.tw = tw_for_kernel_len(l)
        self.darker = (l // 4) % 2 == 0
        self.poison = poison_for(self.darker)
        self.radii = (ws[0] // 2, ws[1] // 2)
        rng = np.random.default_rng([l, ws[0], ws[1], h, w, nf, len(content)])
        if content == "fill":                  # levels around the fill: the DC level is the fill
            self.fill = 128
            frames = (128 + rng.integers(-2, 3, (nf, h, w))).astype(np.uint8)
        elif content == "empty":               # nothing to find but, inside the frame, an exact tie (below): the refinement decides
            self.fill = 128
            frames = (128 + rng.integers(-2, 3, (nf, h, w))).astype(np.uint8)
        else:                                  # "local dc": levels 25 / 55 under fill 200, the DC level is sampled
            assert content == "local dc"
            self.fill = 200
            frames = np.where(rng.integers(0, 2, (nf, h, w)) == 1, 55, 25).astype(np.uint8)
        rad = max(2, int(self.tw) // 2)
        yy, xx = np.ogrid[0:h, 0:w]
        self.centres = []
        windows = []
        r1, r2 = self.radii
        for k in range(nf):
            ci, cj = h // 2 + 1 + int(rng.integers(-3, 4)), (w // 2 + 1 if col is None else col) + int(rng.integers(-3, 4))      # 1-based
            if content != "empty":
                frames[k][(yy - (ci - 1)) ** 2 + (xx - (cj - 1)) ** 2 <= rad * rad] = self.poison
            else:
                # a 2 x 2 block of the target's colour on a flat patch that reaches l/2 + 2 beyond it: its four pixels see the
                # same neighbourhood, their responses tie mathematically, and no noise level can withdraw the flag (the
                # noise-only windows may be flagged and let go again once the window's own max |pixel - dc| is known)
                # (rows ci, ci + 1 and columns cj, cj + 1, 1-based).  A second block sits in the bottom-right corner, where the
                # tile hangs over the frame and the fill (128 as well) continues the patch: exact_pixel's border path.
                p = l // 2 + 2
                for bi, bj in ((ci, cj), (h - 4, w - 5)):
                    frames[k][max(bi - 1 - p, 0):bi + 1 + p, max(bj - 1 - p, 0):bj + 1 + p] = 128
                for bi, bj in ((ci, cj), (h - 4, w - 5)):
                    frames[k][bi - 1:bi + 1, bj - 1:bj + 1] = self.poison
            self.centres.append((ci, cj))
            per = [(ci + 2, cj - 3),                                   # on the disc
                   (3, w // 2 + 7), (h - 2, w // 2 - 5),               # over the top / bottom border
                   (h // 2 + 3, 4), (h // 2 - 4, w - 3),               # over the left / right border
                   (2, 3), (h - 1, w - 2),                             # over the top-left / bottom-right corner
                   (ci + 1, max(cj + 1 - r2, 2 - l // 2))]             # the target in the window's last columns (the fold column)
            windows += [(k, g) for g in per]
        self.frames = frames
        self.per_frame = len(windows) // nf
        order = rng.permutation(len(windows))
        self.windows = [windows[i] for i in order] + [windows[order[0]], windows[order[1]]]       # (repeats)
        assert [k for k, _ in self.windows] != sorted(k for k, _ in self.windows)
        self.by_frame = [[g for k, g in windows if k == f] for f in range(nf)]                   # frame_index None: window b on frame b
        self._ref = {}

    def interior(self, g):
        """The window's padded tile (its columns rounded up to whole dwords) lies inside the frame."""
        hw, (r1, r2) = self.l // 2, self.radii
        i0, j0 = g[0] - r1 - hw - 1, g[1] - r2 - hw - 1
        tw4 = (2 * r2 + self.l + 3) // 4 * 4
        return i0 >= 0 and j0 >= 0 and i0 + 2 * r1 + self.l <= self.h and j0 + tw4 <= self.w

    def kernel(self, oracle):
        if "K" not in self._ref:
            self._ref["K"] = oracle.dog_kernel(oracle.sigma(self.tw), self.darker)
            assert self._ref["K"].shape[0] == self.l
        return self._ref["K"]

    def position(self, oracle, k, g, frames=None, tag=None):
        """The oracle's position for guess g on frame k of `frames` (contiguous; None: the scene's own), memoised per `tag`
        — the name of the frames, None for the scene's own."""
        assert (frames is None) == (tag is None)
        key = (tag, k, int(g[0]), int(g[1]))
        if key not in self._ref:
            f = self.frames if frames is None else frames
            self._ref[key] = tuple(oracle.detect(f[k], self.fill, self.kernel(oracle), self.radii, (int(g[0]), int(g[1]))))
        return self._ref[key]

    def worst(self):
        """The worst corner of the layout matrix: odd slack, odd base, odd gap."""
        return make(self.frames, 19, 2 * self.w + 5, 3 * self.w + 7, self.poison)


# name -> (kernel length, window, frame h, w, frames, the target's column or None for the frame's centre)
SCENES = {
    "l29 21x21":        (29, (21, 21), 96, 128, 3, None),     # ring 20, fused, two-pass l = 29, chains
    "l29 21x21 odd w":  (29, (21, 21), 96, 127, 3, None),     # the full matrix: slack 0 needs an odd width
    "l17 33x45":        (17, (33, 45), 96, 128, 3, None),     # roll 117
    "l65 45x45":        (65, (45, 45), 200, 240, 3, None),    # roll 100 (one partial strip), ring 0 … 13, two-pass plain
    "l65 45x65":        (65, (45, 65), 200, 240, 3, None),    # roll 100: a single remainder column (thin kernel, fold)
    "l65 45x131":       (65, (45, 131), 200, 240, 3, None),   # roll 100: two strips plus thin columns
    "l65 45x513":       (65, (45, 513), 200, 300, 3, 240),      # roll 100: eight strips and one column, folded without being asked
    "l101 45x45":       (101, (45, 45), 200, 240, 3, None),   # roll 201, two-pass blocked
    "l65 129x129":      (65, (129, 129), 200, 240, 3, None),     # tiled
}
CONTENTS = ("fill", "local dc")
USED = [(name, c) for name in SCENES for c in CONTENTS + ("empty",)]      # "empty": exact mode, and the raw FP32 ranking of exact ties
_CACHE = {}


def scene(name, content="fill"):
    if (name, content) not in _CACHE:
        l, ws, h, w, nf, per = SCENES[name]
        _CACHE[(name, content)] = Scene(l, ws, h, w, nf, content, per)
    return _CACHE[(name, content)]


# ---- the layout matrix ----
SLACKS = (1, 3, 19, 64)            # plus 0 with an odd w
BASES = (0, 1, 2, 3, 5, 7, 13)     # base mod 16


def matrix(sc):
    """Every (slack, base, gap) of the matrix for a scene (slack 0 only where its width is odd)."""
    slacks = SLACKS + ((0,) if sc.w % 2 else ())
    return [(s, 32 + b, g) for s in slacks for b in BASES for g in (0, 7, 3 * sc.w + 7)]


def diagonal(sc):
    """A diagonal of the matrix that ends in its worst corner (odd slack, odd base, odd gap)."""
    return [(1, 32 + 1, 7), (3, 32 + 2, 0), (64, 32 + 13, 7), (1, 32, 3 * sc.w + 7), (19, 2 * sc.w + 5, 3 * sc.w + 7)]


def overlap_of(sc, slack=19, base=32 + 7):
    """The scene's frames as overlapping rows of one tall image (step = 2h/3), and as nf aliases of its frame 0.  The
    contiguous twin — np.ascontiguousarray(view) — is what the oracle is asked about."""
    step = 2 * sc.h // 3
    tall = np.concatenate([sc.frames[0]] + [sc.frames[k][sc.h - step:] for k in range(1, sc.nf)])
    return overlapping(tall, sc.nf, sc.h, step, slack, base, sc.poison)


def alias_of(sc, slack=3, base=32 + 5):
    return aliased(sc.frames[0], sc.nf, slack, base, sc.poison)
