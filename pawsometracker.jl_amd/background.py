"""A static background model on device-resident frames (pdog_bg_*; this library's addition, include/pawsome_background.h
states the rule): the per-pixel LOWER MEDIAN of some frames of a stack — the value at rank (K - 1) // 2 of the K sample
values sorted ascending — and frames of the stack with that model subtracted, clamp(128 + frame - model, 0, 255), for the
chains to walk instead of the raw grey levels.  Furniture that is part of every frame is part of the median and not of the
subtracted frames; the difference keeps its sign, so `darker_target` keeps its meaning.

    with Background(h, w) as bg:
        bg.estimate(frames, background_samples(table, 25))
        sub = bg.subtract(frames, table)          # uint8 cuda [len(table), h, w]

track_video(..., background=K) does this in chunks, without ever holding more than `background_chunk` subtracted frames.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._args import background_k, device_frames, host_samples, host_steps

BG_MAX_SAMPLES = _lib.BG_MAX_SAMPLES    # PDOG_BG_MAX_SAMPLES


def background_samples(table, k):
    """The sample rule (pdog_bg_samples, host arithmetic): of a table of m frame indices the k' = min(k, m) entries
    table[i * m // k'], i = 0 ... k'-1, numpy int32.  k: 1 ... 64."""
    table = host_steps(table, "table")
    k = background_k(k)
    if len(table) < 1:
        raise ValueError("table: no frame to sample")
    out = np.empty(min(k, len(table)), np.int32)
    n = C.c_int()
    _lib.check(_lib.lib().pdog_bg_samples(C.c_void_p(table.ctypes.data), len(table), k, C.c_void_p(out.ctypes.data), len(out), C.byref(n)))
    return out[:n.value]


class Background(_lib.Handle):
    """The model of one frame size on one device (pdog_bg).  Every method runs on torch's current stream, with no host
    synchronisation; the model is carried in stream order."""

    def __init__(self, frame_h, frame_w, device=0):
        for name, v in (("frame_h", frame_h), ("frame_w", frame_w)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, not {type(v).__name__}")
            if v < 1:
                raise ValueError(f"{name}: {v} is not a positive size")
        self._hw = (int(frame_h), int(frame_w))
        self.device = int(device)
        super().__init__(_lib.new_handle(_lib.lib().pdog_bg_create, self.device, *self._hw), "pdog_bg_destroy")

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def estimate(self, frames, samples):
        """The model becomes the lower median of frames[samples]: frames uint8 cuda [n_frames, h, w] (row stride may exceed w),
        samples 1 ... 64 host integers (a frame named twice counts twice; an entry outside 0 ... n_frames-1 is refused by the
        library, PdogError, before anything is launched).  Returns self."""
        device_frames(frames, "frames", 3, self._hw, self.device)
        s = host_samples(samples, "samples")
        _lib.check(_lib.lib().pdog_bg_estimate(self._h, self._stream(), C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                               frames.shape[0], C.c_void_p(s.ctypes.data), len(s)))
        return self

    def set(self, image):
        """The model becomes a caller's image, e.g. the empty arena: uint8 cuda [h, w] (row stride may exceed w).  Returns self."""
        device_frames(image, "image", 2, self._hw, self.device)
        _lib.check(_lib.lib().pdog_bg_set(self._h, self._stream(), C.c_void_p(image.data_ptr()), image.stride(0)))
        return self

    def image(self):
        """A copy of the model, uint8 cuda [h, w] (PdogError before any estimate or set)."""
        import torch
        out = torch.empty(self._hw, dtype=torch.uint8, device=torch.device("cuda", self.device))
        _lib.check(_lib.lib().pdog_bg_get(self._h, self._stream(), C.c_void_p(out.data_ptr()), out.stride(0)))
        return out

    def subtract(self, frames, frame_table, out=None):
        """out[k] = clamp(128 + frames[frame_table[k]] - model, 0, 255): frames as for estimate, frame_table host integers
        [n_steps] (judged by the library like the overlay's table), out None or a uint8 cuda tensor [n_steps, h, w] whose last
        stride is 1 — bytes between w and its row stride are not written.  Returns out."""
        import torch
        device_frames(frames, "frames", 3, self._hw, self.device)
        table = host_steps(frame_table, "frame_table")
        ns = len(table)
        if out is None:
            out = torch.empty((ns,) + self._hw, dtype=torch.uint8, device=frames.device)
        device_frames(out, "out", 3, self._hw, self.device)
        if out.shape[0] != ns:
            raise ValueError(f"out: {out.shape[0]} frames for {ns} steps")
        _lib.check(_lib.lib().pdog_bg_subtract_indexed(self._h, self._stream(), C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                                       frames.shape[0], C.c_void_p(table.ctypes.data), ns, C.c_void_p(out.data_ptr()),
                                                       out.stride(0), out.stride(1)))
        return out
