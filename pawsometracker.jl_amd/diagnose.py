"""The reference's diagnostic overlay (src/diagnose.jl) on device-resident frames (pdog_diag_*).

`Diagnose(darker_target)(frames, ij)` draws, for each frame, what the reference's `dia(img, point)` (:30-38) puts
in its 360 x 640 buffer before the writer encodes it: the resized frame, the dot at the scaled position and the path
of the last 100 scaled positions, in the target colour.  The label is not drawn and no video is written: the caller
gets the buffers (uint8 cuda [n, 360, 640]) and encodes them however it likes.  The trace runs on from call to call,
at any frame size, like one `Diagnose` across the files of track(files; ...) (:201-207).
"""
import ctypes as C

from . import _lib
from ._args import device_array, device_frames

DIAG_SIZE = (360, 640)     # DIAGNOSTIC_VIDEO_SIZE, src/diagnose.jl:2


def diag_point(frame_h, frame_w, ij):
    """:31: the position scaled into the buffer, round.(ij .* (360 / h, 640 / w)) (ij clamped into the frame first)."""
    src = (C.c_int32 * 2)(int(ij[0]), int(ij[1]))
    out = (C.c_int32 * 2)()
    _lib.check(_lib.lib().pdog_diag_point(int(frame_h), int(frame_w), src, out))
    return int(out[0]), int(out[1])


class Diagnose(_lib.Handle):
    """`struct Diagnose` (:5-23) minus label and writer: the colour (:17) and a trace that lives on the device."""

    def __init__(self, darker_target=True, device=0):
        self.device = int(device)
        self.darker_target = bool(darker_target)
        super().__init__(_lib.new_handle(_lib.lib().pdog_diag_create, self.device, int(self.darker_target)), "pdog_diag_destroy")

    def __call__(self, frames, ij, out=None):
        """frames: uint8 cuda [n, h, w] of any frame size (row stride may exceed w); ij: int32 cuda [n, 2], 1-based
        (row, col), e.g. what BatchTracker.detect_chain returned.  Returns uint8 cuda [n, 360, 640].  Runs on torch's current
        stream (the caching allocator then keeps frames and ij alive for the kernels), with no host synchronisation."""
        import torch
        n, h, w = device_frames(frames, "frames", 3).shape
        device_array(ij, "ij", torch.int32, (n, 2))
        if out is None:
            out = torch.empty((n,) + DIAG_SIZE, dtype=torch.uint8, device=frames.device)
        device_array(out, "out", torch.uint8, (n,) + DIAG_SIZE)
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(_lib.lib().pdog_diag_render(self._h, C.c_void_p(stream), C.c_void_p(frames.data_ptr()), frames.stride(0),
                                               frames.stride(1), h, w, n, C.c_void_p(ij.data_ptr()),
                                               C.c_void_p(out.data_ptr())))
        return out
