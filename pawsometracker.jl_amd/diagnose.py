"""The reference's diagnostic overlay (src/diagnose.jl) on device-resident frames (pdog_diag_*).

`Diagnose(darker_target)(frames, ij)` draws, for each frame, what the reference's `dia(img, point)` (:30-38) puts
in its 360 x 640 buffer before the writer encodes it: the resized frame, the dot at the scaled position and the path
of the last 100 scaled positions, in the target colour.  The label is not drawn and no video is written: the caller
gets the buffers (uint8 cuda [n, 360, 640]) and encodes them however it likes.  The trace runs on from call to call,
at any frame size, like one `Diagnose` across the files of track(files; ...) (:201-207).
"""
import ctypes as C

from . import _lib

DIAG_SIZE = (360, 640)     # DIAGNOSTIC_VIDEO_SIZE, src/diagnose.jl:2


def diag_point(frame_h, frame_w, ij):
    """:31: the position scaled into the buffer, round.(ij .* (360 / h, 640 / w)) (ij clamped into the frame first)."""
    src = (C.c_int32 * 2)(int(ij[0]), int(ij[1]))
    out = (C.c_int32 * 2)()
    _lib.check(_lib.lib().pdog_diag_point(int(frame_h), int(frame_w), src, out))
    return int(out[0]), int(out[1])


class Diagnose:
    """`struct Diagnose` (:5-23) minus label and writer: the colour (:17) and a trace that lives on the device."""

    def __init__(self, darker_target=True, device=0):
        self.device = int(device)
        self.darker_target = bool(darker_target)
        h = C.c_void_p()
        _lib.check(_lib.lib().pdog_diag_create(self.device, int(self.darker_target), C.byref(h)))
        self._h = h

    def __call__(self, frames, ij, out=None):
        """frames: uint8 cuda [n, h, w] (row stride may exceed w); ij: int32 cuda [n, 2], 1-based (row, col), e.g. what
        BatchTracker.detect_chain returned.  Returns uint8 cuda [n, 360, 640].  Runs on torch's current stream (the
        caching allocator then keeps frames and ij alive for the kernels), with no host synchronisation."""
        import torch
        assert self._h, "Diagnose is closed"
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 3 and frames.stride(2) == 1
        assert ij.is_cuda and ij.dtype == torch.int32 and ij.is_contiguous() and ij.shape == (frames.shape[0], 2)
        n, h, w = frames.shape
        if out is None:
            out = torch.empty((n,) + DIAG_SIZE, dtype=torch.uint8, device=frames.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (n,) + DIAG_SIZE
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(_lib.lib().pdog_diag_render(self._h, C.c_void_p(stream), C.c_void_p(frames.data_ptr()), frames.stride(0),
                                               frames.stride(1), h, w, n, C.c_void_p(ij.data_ptr()),
                                               C.c_void_p(out.data_ptr())))
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().pdog_diag_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
