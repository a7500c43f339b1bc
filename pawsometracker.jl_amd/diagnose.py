"""The reference's diagnostic overlay (src/diagnose.jl) on device-resident frames (pdog_diag_*).

`Diagnose(darker_target)(frames, ij)` draws, for each frame, what the reference's `dia(img, point)` (:30-38) puts
in its 360 x 640 buffer before the writer encodes it: the resized frame, the dot at the scaled position and the path
of the last 100 scaled positions, in the target colour.  The label is not drawn and no video is written: the caller
gets the buffers (uint8 cuda [n, 360, 640]) and encodes them however it likes.  The trace runs on from call to call,
at any frame size, like one `Diagnose` across the files of track(files; ...) (:201-207).

`Diagnose.render_indexed(frames, frame_table, ij)` draws the same over a frame table — output k is frame frame_table[k] of
one stack, what BatchTracker.detect_chains_indexed walked — and for several targets at once (`set_targets`): every target
has its own trace, all are drawn onto the same buffers (include/pawsome_overlay.h).  Several targets per video are this
library's addition; the reference has one.
"""
import ctypes as C

from . import _lib
from ._args import device_array, device_frames, device_positions, host_steps

DIAG_SIZE = (360, 640)     # DIAGNOSTIC_VIDEO_SIZE, src/diagnose.jl:2
DIAG_MAX_TARGETS = _lib.DIAG_MAX_TARGETS   # PDOG_DIAG_MAX_TARGETS: the traces one handle can carry


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

    def set_targets(self, n):
        """The number of traces the handle carries, 1 ... 1024 (pdog_diag_set_targets).  Empties every trace, also when n is
        the current number."""
        n = int(n)
        if not 1 <= n <= _lib.DIAG_MAX_TARGETS:
            raise ValueError(f"n_targets: {n} is outside 1 ... {_lib.DIAG_MAX_TARGETS}")
        _lib.check(_lib.lib().pdog_diag_set_targets(self._h, n))

    @property
    def targets(self):
        n = C.c_int()
        _lib.check(_lib.lib().pdog_diag_get_targets(self._h, C.byref(n)))
        return n.value

    def render_indexed(self, frames, frame_table, ij, out=None):
        """frames: uint8 cuda [n_frames, h, w], ONE stack (row stride may exceed w); frame_table: host integers [n_steps], the
        frame of each output (entries outside 0 ... n_frames-1 are refused by the library, PdogError, before anything is
        launched); ij: int32 cuda [n_targets, n_steps, 2], 1-based (row, col), n_targets the handle's — what
        BatchTracker.detect_chains_indexed returned, or a column slice out[:, k0:k1] of it as it lies (no copy).  Returns
        uint8 cuda [n_steps, 360, 640]: output k is frame frame_table[k] resized, with every target's dot and the path of
        its last 100 points.  Runs on torch's current stream like __call__, with no host synchronisation."""
        import torch
        n, h, w = device_frames(frames, "frames", 3).shape
        table = host_steps(frame_table, "frame_table")
        ns = len(table)
        stride = device_positions(ij, "ij", ns, frames.device.index)
        if out is None:
            out = torch.empty((ns,) + DIAG_SIZE, dtype=torch.uint8, device=frames.device)
        device_array(out, "out", torch.uint8, (ns,) + DIAG_SIZE, frames.device.index)
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(_lib.lib().pdog_diag_render_indexed(self._h, C.c_void_p(stream), C.c_void_p(frames.data_ptr()), frames.stride(0),
                                                       frames.stride(1), h, w, n, C.c_void_p(table.ctypes.data), ns,
                                                       C.c_void_p(ij.data_ptr()), stride, ij.shape[0], C.c_void_p(out.data_ptr())))
        return out
