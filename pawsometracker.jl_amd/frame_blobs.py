"""Every connected blob of a whole frame, labelled on the GPU (pdog_fb_*, pdog_frame_blobs; this library's addition,
include/pawsome_frame_blobs.h states the rule): the mask is the pixels whose contrast against a grey level reaches
`min_contrast`, the blobs are its connected components, and every blob with min_area <= n <= max_area yields twelve int64
words — n, Sy, Sx, Syy, Syx, Sxx, rmin, rmax, cmin, cmax, first, Ss, rows and columns 0-based — listed in ascending `first`,
the order scipy.ndimage.label numbers them in.

    with FrameBlobs(h, w) as fb:
        count, words = fb.find(subtracted_frames)                 # level 128: what Background.subtract leaves static things at
        n = int(min(count[0, 0], words.shape[1]))
        row, col, theta, major, minor, width = frame_blobs_derive(words[0, :n]).T

track_video(..., n_targets=K, find="frame") starts its targets from these blobs instead of the centre window's peaks.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._args import device_frames, frame_blobs_args, host_steps

FB_WORDS = _lib.FB_WORDS    # PDOG_FB_WORDS


def frame_blobs_derive(words):
    """The derived values of blobs (pdog_frame_blobs_derive, host arithmetic): words — a sequence, a numpy array or a tensor
    [..., 12] of integers as FrameBlobs.find returns them — becomes numpy float64 [..., 6]: the centroid's row and column,
    1-BASED like every position of this library, then theta, the major and minor axes and the equivalent width as shape_derive
    gives them.  A row with n <= 0 (the rows behind a step's count) gives NaN."""
    if hasattr(words, "detach"):
        words = words.detach().cpu().numpy()
    a = np.asarray(words)
    if a.dtype.kind not in "iu":
        raise TypeError(f"words must hold integers, not {a.dtype}")
    if a.ndim < 1 or a.shape[-1] != FB_WORDS:
        raise ValueError(f"words: shape {a.shape}, expected (..., {FB_WORDS})")
    flat = np.ascontiguousarray(a, dtype=np.int64).reshape(-1, FB_WORDS)
    out = np.empty((len(flat), 6), np.float64)
    fn = _lib.lib().pdog_frame_blobs_derive
    for k in range(len(flat)):
        _lib.check(fn(C.c_void_p(flat[k].ctypes.data), C.c_void_p(out[k].ctypes.data)))
    return out.reshape(a.shape[:-1] + (6,))


def frame_start_guesses(words, k):
    """The start rule of track_video(find="frame") on a step's kept blobs, words [n, 12]: the k blobs of largest n, ties to the
    lower `first`, largest first, as [(row, col)] — their centroids (frame_blobs_derive: 1-based), rounded half to even."""
    words = np.asarray(words, dtype=np.int64).reshape(-1, FB_WORDS)
    order = sorted(range(len(words)), key=lambda i: (-int(words[i, 0]), int(words[i, 10])))[:k]
    rc = frame_blobs_derive(words[order])[:, :2]
    return [(int(np.rint(r)), int(np.rint(c))) for r, c in rc]


def frame_size_refusal(frame_h, frame_w):
    """The admitted frame sizes (include/pawsome_frame_blobs.h, "Sizes"; size_refusal in csrc/pdog_frame_blobs.hpp) in Python
    integers: None for a size the rule admits, otherwise what of it does not fit.  h, w >= 1, h * w <= 2^30,
    w <= PDOG_MAX_ROW_STRIDE, and the words of the one blob of a full mask — Syy = w * S2(h), Sxx = h * S2(w),
    Syx = T(h) * T(w), S2(k) = (k-1)k(2k-1)/6, T(k) = k(k-1)/2 — at most 2^63 - 1."""
    h, w, most = int(frame_h), int(frame_w), 2**63 - 1
    s2, t = (lambda k: (k - 1) * k * (2 * k - 1) // 6), (lambda k: k * (k - 1) // 2)
    if h < 1 or w < 1:
        return "a side is not positive"
    if h * w > 2**30:
        return "more than 2^30 pixels"
    if w > _lib.PDOG_MAX_ROW_STRIDE:
        return "frame_w exceeds PDOG_MAX_ROW_STRIDE"
    if w * s2(h) > most:
        return "Syy of a full frame leaves 63 bits"
    if h * s2(w) > most:
        return "Sxx of a full frame leaves 63 bits"
    if t(h) * t(w) > most:
        return "Syx of a full frame leaves 63 bits"
    return None


class FrameBlobs(_lib.Handle):
    """The scratch of one frame size on one device (pdog_fb): 8 bytes per pixel and step in flight.  find() runs on torch's
    current stream, with no host synchronisation.  The sizes admitted are those whose full-frame sums fit an int64
    (frame_size_refusal): at most 2^30 pixels, frame_w <= PDOG_MAX_ROW_STRIDE = 2^21, and w * S2(h), h * S2(w) and T(h) * T(w)
    at most 2^63 - 1 — 3 024 617 rows of one pixel, 243 353 rows of 1920, 3 rows of 2^21; ValueError beyond."""

    def __init__(self, frame_h, frame_w, device=0, steps_in_flight=8):
        for name, v in (("frame_h", frame_h), ("frame_w", frame_w), ("steps_in_flight", steps_in_flight)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, not {type(v).__name__}")
            if v < 1:
                raise ValueError(f"{name}: {v} is not a positive number")
        if steps_in_flight > _lib.FB_MAX_IN_FLIGHT:
            raise ValueError(f"steps_in_flight: {steps_in_flight} lies outside 1 ... {_lib.FB_MAX_IN_FLIGHT}")
        why = frame_size_refusal(frame_h, frame_w)
        if why:
            raise ValueError(f"frames of {frame_h} x {frame_w} are not admitted: {why}")
        self._hw = (int(frame_h), int(frame_w))
        self.device = int(device)
        self.steps_in_flight = int(steps_in_flight)
        super().__init__(_lib.new_handle(_lib.lib().pdog_fb_create, self.device, *self._hw, self.steps_in_flight), "pdog_fb_destroy")

    def find(self, frames, table=None, level=128, darker_target=True, min_contrast=8, connectivity=8, min_area=1, max_area=None, cap=64):
        """The blobs of frames[table[k]] for every step k: frames uint8 cuda [n_frames, h, w] (row stride may exceed w), table
        None (every frame in turn) or host integers [n_steps] (a frame may be named twice; an entry outside the stack is refused
        by the library, PdogError, before anything is launched).  A pixel p is in the mask when level - p >= min_contrast
        (darker_target) or p - level >= min_contrast; connectivity is 4 or 8; blobs with min_area <= n <= max_area (None: no
        upper limit) are kept.  Returns (count, words): count int32 cuda [n_steps, 2] — the number of kept blobs and the mask's
        pixel count —, words int64 cuda [n_steps, cap, 12] — the first `cap` kept blobs in ascending `first`, zero behind
        min(count, cap).  More steps than steps_in_flight run in rounds inside the one call."""
        import torch
        args = frame_blobs_args(self._hw[0] * self._hw[1], level, darker_target, min_contrast, connectivity, min_area, max_area, cap)
        if not isinstance(frames, torch.Tensor) or frames.dim() != 3:
            raise TypeError("frames must be a uint8 cuda tensor [n, h, w]")
        steps = np.arange(frames.shape[0], dtype=np.int32) if table is None else host_steps(table, "table")
        device_frames(frames, "frames", 3, self._hw, self.device)
        ns, cap = len(steps), args[-1]
        dev = torch.device("cuda", self.device)
        count = torch.empty((ns, 2), dtype=torch.int32, device=dev)
        words = torch.empty((ns, cap, FB_WORDS), dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib().pdog_frame_blobs(self._h, stream, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                               frames.shape[0], C.c_void_p(steps.ctypes.data), ns, *args[:-1], cap,
                                               C.c_void_p(words.data_ptr()), C.c_void_p(count.data_ptr())))
        return count, words
