"""Host-side mirror of the reference `Tracker` on top of the C ABI.

Same spellings as /root/reference/src/PawsomeTracker.jl so that call sites
(:94-95, :103-105, :166-167) and the parity tests read like the reference:

    trckr = Tracker(img, target_width, window_size, darker_target)   # :39-52
    trckr.img.data[...] = next_frame                                  # :166
    ij = trckr(guess)                                                 # :55-62

The arithmetic runs in the HIP library (libpawsome_dog.so); this file holds no
filter code and never imports oracle/.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._args import host_i32


def get_sigma(target_width):
    """src/PawsomeTracker.jl:30"""
    return _lib.lib().pdog_sigma(float(target_width))


def guess_window_size(target_width):
    """src/PawsomeTracker.jl:64-68"""
    return _lib.lib().pdog_default_window(float(target_width))


def fix_window_size(window_size):
    """src/PawsomeTracker.jl:70-72: (w, h) -> (h, w); Int -> (l, l)"""
    if isinstance(window_size, (tuple, list)):
        w, h = window_size
        return (int(h), int(w))
    return (int(window_size), int(window_size))


DEFAULT_STOP = _lib.DEFAULT_STOP        # DEFAULT_MAX_DURATION_SECONDS, src/PawsomeTracker.jl:19


def time_axis(start, stop, fps, first=None):
    """ts of src/PawsomeTracker.jl:150-152 (pdog_time_axis): n = round(Int, fps * (stop - start)) stamps from start to
    stop, numpy float64.  Last-bit equality with Julia's range is unpinned (include/pawsome_video.h).  first = m: only
    ts[:m] (:173) — the library reports n, and the m stamps are formed as it forms them, start + j * ((stop - start) / (n - 1))
    in Float64, without the other n - m (the default stop is a day away: two million stamps at 24 per second)."""
    start, stop, fps = float(start), float(stop), float(fps)
    n = C.c_int()
    _lib.check(_lib.lib().pdog_time_axis(start, stop, fps, None, 0, C.byref(n)))
    if first is not None and 0 <= first < n.value and n.value > 1:
        return start + np.arange(int(first), dtype=np.float64) * ((stop - start) / float(n.value - 1))
    ts = np.empty(n.value, np.float64)
    _lib.check(_lib.lib().pdog_time_axis(start, stop, fps, C.c_void_p(ts.ctypes.data), n.value, C.byref(n)))
    return ts if first is None else ts[:max(int(first), 0)]


def fps_table(rate, n_frames, start=0, stop=DEFAULT_STOP, fps=24):
    """The frames `ffmpeg -ss start -i f -t stop-start -vf fps=fps` (src/PawsomeTracker.jl:155) selects from a stack of
    n_frames frames at `rate` frames per second (pdog_fps_table), numpy int32: one frame index per output that exists.
    The rule is a recollection of libavfilter's fps filter, unpinned (include/pawsome_video.h): a caller who knows better
    builds their own table for BatchTracker.detect_chains_indexed."""
    args = (float(rate), int(n_frames), float(start), float(stop), float(fps))
    n = C.c_int()
    _lib.check(_lib.lib().pdog_fps_table(*args, None, 0, C.byref(n)))
    table = np.empty(n.value, np.int32)
    _lib.check(_lib.lib().pdog_fps_table(*args, C.c_void_p(table.ctypes.data), n.value, C.byref(n)))
    return table


def mode(img):
    """mode(_img), src/PawsomeTracker.jl:47 (StatsBase tie rule, column-major scan)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise TypeError("frame must be a 2-D uint8 (GRAY8) array")
    if not img.flags.c_contiguous:
        img = np.ascontiguousarray(img)
    out = C.c_int()
    _lib.check(_lib.lib().pdog_mode_u8(img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], C.byref(out)))
    return out.value


def subpixel(resp5, ij):
    """The sub-pixel rule (pdog_subpixel; this library's addition, not the reference's): resp5 = the response
    {c, up, down, left, right} at the 1-based position ij and its four neighbours -> (row, col) floats.  Per axis the
    vertex of the parabola through the three values, within half a pixel of ij; ij itself where it is no strict maximum."""
    r = (C.c_double * 5)(*[float(v) for v in resp5])
    src = (C.c_int32 * 2)(int(ij[0]), int(ij[1]))
    out = (C.c_double * 2)()
    _lib.check(_lib.lib().pdog_subpixel(r, src, out))
    return float(out[0]), float(out[1])


def _host(v, dtype):
    """A tensor, array or sequence as a contiguous host array of `dtype`."""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=dtype)


def shape_derive(sums, ij):
    """Step 7 of the shape rule on the host (pdog_shape_derive; include/pawsome_shape.h): sums — the eight integers
    (n, Sy, Sx, Syy, Syx, Sxx, b, c) BatchTracker.shapes(want_sums=True) returns, [8] or [n, 8] — and ij, the 1-based
    positions they were taken at (clamped into the frame), [2] or [n, 2] -> numpy float64 [6] or [n, 6]: row, col, theta,
    major, minor, width; NaN where n is 0."""
    s, p = _host(sums, np.int32), _host(ij, np.int32)
    if s.shape[-1:] != (8,) or s.ndim not in (1, 2):
        raise ValueError(f"sums: shape {s.shape}, expected (8,) or (n, 8)")
    if p.shape != s.shape[:-1] + (2,):
        raise ValueError(f"ij: shape {p.shape}, expected {s.shape[:-1] + (2,)}")
    s2, p2 = s.reshape(-1, 8), p.reshape(-1, 2)
    out = np.empty((len(s2), 6), np.float64)
    fn = _lib.lib().pdog_shape_derive
    for k in range(len(s2)):
        _lib.check(fn(C.c_void_p(s2[k].ctypes.data), C.c_void_p(p2[k].ctypes.data), C.c_void_p(out[k].ctypes.data)))
    return out.reshape(s.shape[:-1] + (6,))


def headings(shape_or_theta, indices, min_step=1.0):
    """Step 8 of the shape rule (pdog_shape_headings; include/pawsome_shape.h): theta's 180 degree ambiguity resolved with
    the motion, per target over its steps.  shape_or_theta: the `shape` a track returned, [m, 6] or [n_targets, m, 6], or
    its theta column alone, [m] or [n_targets, m]; indices: the positions, [m, 2] or [n_targets, m, 2].  A step of at least
    min_step pixels points the heading along the motion, a shorter one keeps the side of the previous heading; NaN where
    theta is.  Returns numpy float64 [m] or [n_targets, m], in (-pi, pi], from +col towards +row."""
    if isinstance(min_step, bool) or not isinstance(min_step, (int, float, np.integer, np.floating)):
        raise TypeError(f"min_step must be a real number, not {type(min_step).__name__}")
    if not float(min_step) >= 0:
        raise ValueError(f"min_step: {min_step} is not a distance >= 0")
    ij = _host(indices, np.int32)
    th = _host(shape_or_theta, np.float64)
    if ij.ndim not in (2, 3) or ij.shape[-1] != 2:
        raise ValueError(f"indices: shape {ij.shape}, expected (m, 2) or (n_targets, m, 2)")
    if th.shape == ij.shape[:-1] + (6,):
        th = np.ascontiguousarray(th[..., 2])
    if th.shape != ij.shape[:-1]:
        raise ValueError(f"shape_or_theta: shape {th.shape}, expected {ij.shape[:-1]} or {ij.shape[:-1] + (6,)}")
    out = np.empty(th.shape, np.float64)
    m = th.shape[-1]
    th2, ij2, out2 = th.reshape(-1, m), ij.reshape(-1, m, 2), out.reshape(-1, m)
    for t in range(len(th2)):
        _lib.check(_lib.lib().pdog_shape_headings(C.c_void_p(th2[t].ctypes.data), C.c_void_p(ij2[t].ctypes.data), m, float(min_step),
                                                  C.c_void_p(out2[t].ctypes.data)))
    return out


def _shape_keywords(shape, shape_radius, shape_min_contrast, shape_connectivity=None):
    """The shape keywords of the track functions, judged before anything touches the device: (radius, min_contrast,
    connectivity) as the library takes them — connectivity None: the shape rule, 4 or 8: the blob rule —, or None without
    shape."""
    from ._args import blob_args, shape_args
    if not isinstance(shape, bool):
        raise TypeError("shape must be True or False")
    if not shape:
        if shape_radius is not None or shape_min_contrast is not None:
            raise ValueError("shape_radius and shape_min_contrast belong to shape")
        if shape_connectivity is not None:
            raise ValueError("shape_connectivity belongs to shape")
        return None
    mc = 8 if shape_min_contrast is None else shape_min_contrast
    if shape_connectivity is None:
        return shape_args(shape_radius, mc, "shape_") + (None,)
    return blob_args(shape_radius, mc, shape_connectivity, "shape_")


def _shapes_or_blobs(bt, frames, ij, fi, kw):
    """BatchTracker.shapes, or .blobs where the keywords name a connectivity: float64 cuda [n, 6]."""
    if kw[2] is None:
        return bt.shapes(frames, ij, fi, kw[0] or None, kw[1])
    return bt.blobs(frames, ij, fi, kw[0] or None, kw[1], kw[2])


class _PaddedFrame:
    """Stands in for the PaddedView at :48: `.data` is the live frame buffer the
    caller overwrites in place each frame (:166); everything outside reads as `fillvalue`."""

    def __init__(self, data, fillvalue):
        self.data = data
        self.fillvalue = fillvalue


def _to_device(frame, ij, device):
    """One host frame and one 1-based position as the batch entry points take them: uint8 cuda [1, h, w], int32 cuda [1, 2]."""
    import torch
    dev = torch.device("cuda", device)
    f = torch.from_numpy(np.ascontiguousarray(frame, np.uint8)).to(dev).unsqueeze(0)
    return f, torch.tensor([[int(ij[0]), int(ij[1])]], dtype=torch.int32, device=dev)


class Tracker(_lib.TrackerHandle):
    """src/PawsomeTracker.jl:32-62 — constructor (:39-52) and functor (:55-62)."""

    def __init__(self, img, target_width, window_size, darker_target, device=0):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise TypeError("frame must be a 2-D uint8 (GRAY8) array")
        self.sz = (int(img.shape[0]), int(img.shape[1]))            # :40
        self.radii = (int(window_size[0]) // 2, int(window_size[1]) // 2)  # :44
        self.target_width = float(target_width)
        self.darker_target = bool(darker_target)
        fillvalue = mode(img)                                        # :47
        self.img = _PaddedFrame(np.array(img, dtype=np.uint8, order="C", copy=True), fillvalue)  # :48
        super().__init__(_lib.new_handle(_lib.lib().pdog_create, int(device), self.sz[0], self.sz[1], self.target_width,
                                         int(window_size[0]), int(window_size[1]), int(self.darker_target), fillvalue),
                         "pdog_destroy")
        self.device = int(device)

    # -- the functor, :55-62 --
    def __call__(self, guess, want_resp=False):
        g = (C.c_int32 * 2)(int(guess[0]), int(guess[1]))
        out = (C.c_int32 * 2)()
        data = self.img.data
        resp_ptr = None
        if want_resp:
            info = self.info()
            resp = np.empty((info.win_h, info.win_w), np.float32, order="F")
            resp_ptr = resp.ctypes.data
        _lib.check(_lib.lib().pdog_detect_host(self._h, data.ctypes.data, data.strides[0], g, out, resp_ptr))
        ij = (int(out[0]), int(out[1]))
        return (ij, resp) if want_resp else ij

    def measure(self, ij, want_resp=False):
        """Sub-pixel position (row, col) of the 1-based position ij on the current frame (`img.data`) — and, with
        want_resp, the five responses {c, up, down, left, right} there (pdog_measure).  The frame goes up through torch,
        the kernel runs on the tracker's own stream.  Synchronous, like the functor."""
        import torch
        f, p = _to_device(self.img.data, ij, self.device)
        out = torch.empty((1, 7), dtype=torch.float64, device=f.device)
        torch.cuda.current_stream(f.device).synchronize()     # the upload is on torch's stream
        _lib.check(_lib.lib().pdog_measure(self._h, C.c_void_p(f.data_ptr()), f.stride(0), f.stride(1), 1, None,
                                           C.c_void_p(p.data_ptr()), 1, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(out.data_ptr() + 5 * 8)))
        self.sync()
        v = [float(x) for x in out[0].cpu()]
        return ((v[5], v[6]), tuple(v[:5])) if want_resp else (v[5], v[6])

    def shape(self, ij, radius=None, min_contrast=8, want_sums=False):
        """How the target lies at the 1-based position ij on the current frame (`img.data`): (row, col, theta, major, minor,
        width) as BatchTracker.shapes describes them (pdog_shape) — and, with want_sums, the rule's eight integers.  The
        frame goes up through torch, the kernel runs on the tracker's own stream.  Synchronous, like the functor."""
        import torch
        from ._args import shape_args
        radius, min_contrast = shape_args(radius, min_contrast)
        f, p = _to_device(self.img.data, ij, self.device)
        out = torch.empty((1, 6), dtype=torch.float64, device=f.device)
        sums = torch.empty((1, 8), dtype=torch.int32, device=f.device)
        torch.cuda.current_stream(f.device).synchronize()     # the upload is on torch's stream
        _lib.check(_lib.lib().pdog_shape(self._h, C.c_void_p(f.data_ptr()), f.stride(0), f.stride(1), 1, None,
                                         C.c_void_p(p.data_ptr()), 1, radius, min_contrast, C.c_void_p(sums.data_ptr()),
                                         C.c_void_p(out.data_ptr())))
        self.sync()
        v = tuple(float(x) for x in out[0].cpu())
        return (v, tuple(int(x) for x in sums[0].cpu())) if want_sums else v

    def blob(self, ij, radius=None, min_contrast=8, connectivity=8, want_sums=False):
        """shape() over the connected blob under the position (pdog_blob; include/pawsome_blob.h): (row, col, theta, major,
        minor, width) as BatchTracker.blobs describes them — and, with want_sums, the rule's ten integers.  Synchronous, like
        the functor."""
        import torch
        from ._args import blob_args
        radius, min_contrast, connectivity = blob_args(radius, min_contrast, connectivity)
        f, p = _to_device(self.img.data, ij, self.device)
        out = torch.empty((1, 6), dtype=torch.float64, device=f.device)
        sums = torch.empty((1, 10), dtype=torch.int32, device=f.device)
        torch.cuda.current_stream(f.device).synchronize()     # the upload is on torch's stream
        _lib.check(_lib.lib().pdog_blob(self._h, C.c_void_p(f.data_ptr()), f.stride(0), f.stride(1), 1, None,
                                        C.c_void_p(p.data_ptr()), 1, radius, min_contrast, connectivity,
                                        C.c_void_p(sums.data_ptr()), C.c_void_p(out.data_ptr())))
        self.sync()
        v = tuple(float(x) for x in out[0].cpu())
        return (v, tuple(int(x) for x in sums[0].cpu())) if want_sums else v


def get_guess(start_location, img, sar=1.0):
    """src/PawsomeTracker.jl:74-90: CartesianIndex -> Tuple; (x, y) -> round.((y, x/sar));
    missing (None) -> size(img) .÷ 2.  A CartesianIndex is spelled `("ij", (i, j))` here,
    a bare 2-tuple is (x, y) like the reference's NTuple{2}."""
    if start_location is None:
        return (img.shape[0] // 2, img.shape[1] // 2)          # :86-90
    if isinstance(start_location, tuple) and len(start_location) == 2 and start_location[0] == "ij":
        return (int(start_location[1][0]), int(start_location[1][1]))   # :74-77
    x, y = start_location                                       # :79-84
    return (int(_round_half_even(y)), int(_round_half_even(x / sar)))


def _round_half_even(v):
    return int(np.rint(v))  # Julia's round(Int, x) rounds half to even, like rint


def get_start_ij_and_tracker(start_location, img, target_width, window_size, darker_target, sar=1.0, device=0):
    """src/PawsomeTracker.jl:92-107, both methods."""
    guess = get_guess(start_location, img, sar)
    if start_location is None:                                   # :99-107 auto-detect
        sz = img.shape
        window_size2 = (sz[0] // 4, sz[1] // 4)                  # :102
        trckr = Tracker(img, target_width, window_size2, darker_target, device)   # :103
        ij = trckr(guess)                                        # :104
        trckr.close()
        trckr = Tracker(img, target_width, window_size, darker_target, device)    # :105
        return trckr, ij
    trckr = Tracker(img, target_width, window_size, darker_target, device)        # :94
    return trckr, trckr(guess)                                   # :95


def track_frames(frames, target_width=25, start_location=None, window_size=None, darker_target=True,
                 sar=1.0, device=0, diagnostic=None, subpixel=False, shape=False, shape_radius=None, shape_min_contrast=None,
                 shape_connectivity=None):
    """The frame loop of track_one (src/PawsomeTracker.jl:159-169) on already-decoded GRAY8
    frames (decode stays with the host application): indices[1] from the bootstrap (:161),
    then indices[k] = trckr(indices[k-1]) per frame (:166-167, the intended loop).
    `frames` is an iterable of h x w uint8 arrays.  Returns a list of 1-based (row, col).
    `diagnostic` stands in for the reference's diagnostic_file (:126): None, or a callable that receives, for
    frames 2 ... n in order, the 360 x 640 uint8 numpy buffer dia(img, point) draws (src/diagnose.jl:30-38,
    rendered on the GPU by Diagnose); encoding it is the caller's business.
    With subpixel=True the return value is (indices, sub): sub holds one (row, col) float pair per frame, the first
    frame included — Tracker.measure at each returned position (this library's addition; the indices are unchanged).
    With shape=True the result gains a trailing `shape`, behind sub where that is present: one (row, col, theta, major,
    minor, width) per frame — Tracker.shape at each returned position with shape_radius (None: ceil(target_width)) and
    shape_min_contrast (None: 8); ValueError for either without shape.  Everything else is what it is without the keyword.
    shape_connectivity = 4 or 8 measures `shape` over the connected blob under the position (Tracker.blob; include/pawsome_blob.h)
    instead; None is the shape rule as before; ValueError without shape."""
    shp = _ShapeSink(shape, shape_radius, shape_min_contrast, shape_connectivity)
    sub = [] if subpixel else None
    if diagnostic is None:
        ijs = _track_one(frames, target_width, start_location, window_size, darker_target, sar, device, None, None, sub, shp)
    else:
        from .diagnose import Diagnose
        with Diagnose(darker_target, device) as dia:
            ijs = _track_one(frames, target_width, start_location, window_size, darker_target, sar, device, dia, diagnostic, sub, shp)
    res = (ijs, sub) if subpixel else ijs
    return shp.behind(res)


def track_segments(segments, start_locations=None, target_width=25, window_size=None, darker_target=True,
                   sar=1.0, device=0, diagnostic=None, subpixel=False, shape=False, shape_radius=None, shape_min_contrast=None,
                   shape_connectivity=None):
    """track(files::AbstractVector; ...) (src/PawsomeTracker.jl:181-214) on already-decoded segments: `segments` is a
    list of frame iterables, `start_locations` one start location per segment (default all None).  A None after the
    first segment takes the previous segment's last position (coalesce(loc, end_location), :204-206).  One overlay
    trace spans every segment (one `Diagnose`, :201), across frame sizes.  Returns the concatenated positions — and,
    with subpixel=True, (positions, sub) as track_frames does; with shape=True the trailing `shape` as track_frames does
    (shape_connectivity as there)."""
    shp = _ShapeSink(shape, shape_radius, shape_min_contrast, shape_connectivity)
    segments = list(segments)
    locs = [None] * len(segments) if start_locations is None else list(start_locations)
    if len(locs) != len(segments):
        raise ValueError(f"{len(segments)} segments but {len(locs)} start locations")     # :196
    dia = None
    if diagnostic is not None:
        from .diagnose import Diagnose
        dia = Diagnose(darker_target, device)
    out, end = [], None
    sub = [] if subpixel else None
    try:
        for seg, loc in zip(segments, locs):
            if loc is None and end is not None:
                loc = ("ij", end)                                 # a CartesianIndex, :205
            ijs = _track_one(seg, target_width, loc, window_size, darker_target, sar, device, dia, diagnostic, sub, shp)
            end = ijs[-1]                                         # :206
            out.extend(ijs)
    finally:
        if dia is not None:
            dia.close()
    return shp.behind((out, sub) if subpixel else out)


def _overlay(dia, frame, ij, device):
    """dia(trckr.img.data, indices[k]) for one host frame: it goes up, the 360 x 640 buffer comes back."""
    return dia(*_to_device(frame, ij, device))[0].cpu().numpy()


class _ShapeSink:
    """The shape keywords of track_frames and track_segments: judged at once, then one Tracker.shape per returned position."""

    def __init__(self, shape, shape_radius, shape_min_contrast, shape_connectivity=None):
        self.args = _shape_keywords(shape, shape_radius, shape_min_contrast, shape_connectivity)
        self.rows = []

    def measure(self, trckr, ij):
        if self.args is None:
            return
        if self.args[2] is None:
            self.rows.append(trckr.shape(ij, self.args[0] or None, self.args[1]))
        else:
            self.rows.append(trckr.blob(ij, self.args[0] or None, self.args[1], self.args[2]))

    def behind(self, res):
        """res with the shapes as its last element, if they were asked for."""
        if self.args is None:
            return res
        return (res if isinstance(res, tuple) else (res,)) + (self.rows,)


def _track_one(frames, target_width, start_location, window_size, darker_target, sar, device, dia, diagnostic, sub=None, shp=None):
    if window_size is None:
        window_size = guess_window_size(target_width)            # :136
    window_size = fix_window_size(window_size)                   # :142
    it = iter(frames)
    img = np.asarray(next(it))                                   # :159
    trckr, ij = get_start_ij_and_tracker(start_location, img, target_width, window_size, darker_target, sar, device)
    indices = [ij]
    try:
        if sub is not None:
            sub.append(trckr.measure(ij))                        # (sub: one float pair per frame, appended in place)
        if shp is not None:
            shp.measure(trckr, ij)
        for frame in it:
            trckr.img.data[...] = frame                          # :166
            indices.append(trckr(indices[-1]))                   # :167
            if sub is not None:
                sub.append(trckr.measure(indices[-1]))
            if shp is not None:
                shp.measure(trckr, indices[-1])
            if dia is not None:
                diagnostic(_overlay(dia, trckr.img.data, indices[-1], device))   # :168
    finally:
        trckr.close()
    return indices


def _check_sink(diagnostic, diagnostic_chunk):
    """The overlay keywords of track_video and track_clips, judged before anything touches the device."""
    if diagnostic is not None and not callable(diagnostic):
        raise TypeError("diagnostic must be None or a callable")
    if isinstance(diagnostic_chunk, bool) or not isinstance(diagnostic_chunk, (int, np.integer)):
        raise TypeError("diagnostic_chunk must be an integer")
    if diagnostic_chunk < 1:
        raise ValueError(f"diagnostic_chunk: {diagnostic_chunk} is not a positive number of steps")
    return int(diagnostic_chunk)


def _render_steps(dia, frames, table, ij, chunk, sink):
    """Steps 1 ... len(table)-1 of a chain's result ij [n_targets, len(table), 2] over `table` drawn by `dia` (the bootstrap
    frame is not drawn, src/PawsomeTracker.jl:163-168), at most `chunk` steps at a time into ONE buffer that the next chunk
    overwrites: sink(k0, overlays), overlays[i] belonging to step k0 + i."""
    import torch
    from .diagnose import DIAG_SIZE
    n = len(table)
    if n < 2:
        return
    buf = torch.empty((min(chunk, n - 1),) + DIAG_SIZE, dtype=torch.uint8, device=frames.device)
    for k0 in range(1, n, chunk):
        k1 = min(n, k0 + chunk)
        sink(k0, dia.render_indexed(frames, table[k0:k1], ij[:, k0:k1], out=buf[:k1 - k0]))


def track_clips(frames, target_width=25, start_locations=None, window_size=None, darker_target=True, sar=1.0,
                lengths=None, subpixel=False, diagnostic=None, diagnostic_clips=None, diagnostic_chunk=256):
    """The reference's `track` for every clip of a device-resident stack at once: frames is a uint8 cuda tensor
    [n_clips, n_frames, h, w] (clips stacked contiguously), the device is the tensor's.  Each clip is tracked as its own
    `Tracker` would track it (src/PawsomeTracker.jl:39-52): the fill is the mode of ITS first frame (:47-48), the first
    position comes from ITS bootstrap — the sz .÷ 4 window for a start location of None (:99-107), the functor at the
    given guess otherwise (:92-97) — and the loop continues from the second frame (:161-167).  `start_locations` is None
    or one entry per clip, spelled as for get_guess; `lengths` is None or the number of frames of each clip
    (0 ... n_frames).  Returns int32 cuda [n_clips, n_frames, 2], 1-based (row, col); rows beyond a clip's length hold 0.
    With subpixel=True the result is (indices, sub), sub float64 cuda of the same shape: BatchTracker.measure at every
    returned position under that clip's fill (this library's addition; the indices are unchanged).
    `diagnostic` stands in for the reference's diagnostic_file (:126) as in track_frames, here on the device: None, or a
    callable.  Every clip of `diagnostic_clips` (None: all) is then drawn as a `track` call of its own would draw it, with
    a fresh trace per clip: its frames 2 ... len (the bootstrap frame is not drawn, :163-168; a clip shorter than two frames
    draws nothing), rendered from the stack as it lies, at most `diagnostic_chunk` frames at a time, and handed over as
    diagnostic(clip, k0, overlays): overlays uint8 cuda [<= diagnostic_chunk, 360, 640], overlays[i] belonging to frame
    k0 + i of that clip.  The buffer is reused once the sink returns: the sink consumes it with torch work on the current
    stream, or copies it.  Positions and sub are what they are without the keyword."""
    import torch
    from .batch import BatchTracker
    chunk = _check_sink(diagnostic, diagnostic_chunk)
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4):
        raise TypeError("frames must be a uint8 cuda tensor [n_clips, n_frames, h, w]")
    nc, nf, h, w = (int(v) for v in frames.shape)
    drawn = range(nc) if diagnostic_clips is None else [int(c) for c in diagnostic_clips]
    if any(not 0 <= c < nc for c in drawn):
        raise ValueError(f"diagnostic_clips: clip numbers 0 ... {nc - 1} expected")
    locs = [None] * nc if start_locations is None else list(start_locations)
    if len(locs) != nc:
        raise ValueError(f"{nc} clips but {len(locs)} start locations")
    lens = np.full(nc, nf, np.int32) if lengths is None else host_i32(lengths, "lengths", nc)
    if (lens < 0).any() or (lens > nf).any():
        raise ValueError("lengths: one value in 0 ... n_frames per clip")
    if window_size is None:
        window_size = guess_window_size(target_width)            # :136
    window_size = fix_window_size(window_size)                   # :142
    dev = frames.device
    flat = frames.flatten(0, 1)
    with torch.cuda.device(dev):
        bt = BatchTracker(h, w, target_width, window_size, darker_target, 0, device=dev.index)
        try:
            # 1. the fills, :47: one launch, one read-back of n_clips ints
            first_frame = torch.arange(nc, dtype=torch.int32, device=dev) * nf
            fills = bt.clip_modes(flat, first_frame).cpu().numpy()
            # 2. the first positions, :92-107: one functor application on each clip's first frame
            auto = np.array([loc is None for loc in locs], bool)
            guesses = torch.tensor([get_guess(loc, frames[0, 0], sar) for loc in locs], dtype=torch.int32, device=dev).reshape(nc, 2)
            has = lens >= 1
            out = torch.zeros((nc, nf, 2), dtype=torch.int32, device=dev)    # row 0 of a clip first holds its bootstrap
            if (auto & has).any():
                bt4 = BatchTracker(h, w, target_width, (h // 4, w // 4), darker_target, 0, device=dev.index)   # :102-103
                try:
                    bt4.track_clips(frames, guesses, fills, (auto & has).astype(np.int32), out=out)            # :104
                    bt4.sync()           # a guess outside the padded frame raises here, like the reference's BoundsError
                finally:
                    bt4.close()
            if (~auto & has).any():
                bt.track_clips(frames, guesses, fills, (~auto & has).astype(np.int32), out=out)                # :95
                bt.sync()
            starts = out[:, 0].contiguous()
            # 3. the loop from the second frame on, :161-167
            bt.track_clips(frames, starts, fills, lens, first=1, out=out)
            sub = None
            if subpixel:
                sub = torch.zeros((nc, nf, 2), dtype=torch.float64, device=dev)
                k = np.arange(nf)
                for f in np.unique(fills[has]):
                    clips = np.nonzero(has & (fills == f))[0]
                    idx = np.concatenate([c * nf + k[: lens[c]] for c in clips])
                    fi = torch.from_numpy(idx.astype(np.int32)).to(dev)
                    bt.set_fill(int(f))
                    sub.view(-1, 2)[fi.long()] = bt.measure(flat, out.view(-1, 2)[fi.long()].contiguous(), fi)
            bt.sync()                    # what the kernels raised (PdogError) surfaces before the positions are handed out
            if diagnostic is not None:
                from .diagnose import Diagnose
                with Diagnose(darker_target, dev.index) as dia:     # one handle for all clips
                    for c in drawn:
                        dia.set_targets(1)                           # a fresh trace per clip, as per `track` call (:201)
                        table = c * nf + np.arange(int(lens[c]), dtype=np.int32)
                        _render_steps(dia, flat, table, out[c:c + 1], chunk, lambda k0, ov, c=c: diagnostic(c, k0, ov))
            return (out, sub) if subpixel else out
        finally:
            bt.close()


def track_video(frames, rate, start=0, stop=DEFAULT_STOP, fps=24, target_width=25, start_locations=None, window_size=None,
                darker_target=True, sar=1.0, subpixel=False, diagnostic=None, diagnostic_chunk=256, n_targets=None,
                min_distance=None, find="window", shape=False, shape_radius=None, shape_min_contrast=None, shape_connectivity=None, shape_split=False,
                background=None, background_chunk=256, predict=False, motion=False, coast=None, min_response=None, exclusive=False, min_ratio=None):
    """The reference's `track(file; start, stop, fps, ...)` (src/PawsomeTracker.jl:130-173) on ONE device-resident video at
    its native rate: frames is a uint8 cuda tensor [n_frames, h, w] recorded at `rate` frames per second.  Nothing is
    decoded or copied: fps_table names the frames the reference's ffmpeg line (:155) would hand over, and every target's
    chain walks that table over the shared frames in one indexed call.  `start_locations` is None, one location, or a
    list with one location per target (several animals in one arena), each spelled as for get_guess.  As in the reference
    the fill is the mode of the first SELECTED frame (:159, :47), every target gets its own bootstrap on that frame — the
    sz .÷ 4 window for None (:99-107), the functor at the given guess otherwise (:92-97) — and the loop starts from the
    second selected frame (:161-167).  Returns (ts, indices): ts numpy float64 [m], the time stamps of :150-152 cut to the m
    frames that exist (:173), indices int32 cuda [n_targets, m, 2], 1-based (row, col).  With subpixel=True the result is
    (ts, indices, sub), sub float64 cuda of the same shape: BatchTracker.measure at every position (this library's addition).
    `diagnostic` stands in for the reference's diagnostic_file (:126) as in track_frames, here on the device: None, or a
    callable.  The overlay of the selected frames 2 ... m (the bootstrap frame is not drawn, :163-168) is then rendered
    through the same table, without a copy of the frames, at most `diagnostic_chunk` steps at a time, and handed over as
    diagnostic(k0, overlays): overlays uint8 cuda [<= diagnostic_chunk, 360, 640], overlays[i] belonging to step k0 + i of
    ts and indices.  The buffer is reused once the sink returns: the sink consumes it with torch work on the current
    stream, or copies it.  ALL targets are drawn onto the same overlay, each with its own dot and trace — this library's
    addition: the reference has one target per video.  ts, indices and sub are what they are without the keyword.
    `n_targets` = K (1 ... 32, with start_locations None) FINDS the targets instead: the K starts are the K best, mutually
    separated peaks (BatchTracker.detect_peaks; none closer than `min_distance` pixels to another, None: ceil(target_width))
    of the reference's bootstrap window — sz .÷ 4 around the frame centre on the first selected frame (:99-107) —, in pick
    order: target 0 starts where the reference's own bootstrap puts its one target.  ValueError when fewer than K picks
    have a positive response, or when n_targets comes with start_locations.  Everything after the starts is what a list of
    K start locations gets.
    `find` = "frame" (with n_targets; "window", the default, is the rule above, bit for bit) finds the K starts in the WHOLE first
    selected frame instead (this library's addition; include/pawsome_frame_blobs.h states the rule and the choices): the frame's
    connected blobs (FrameBlobs.find) whose contrast against the level — 128 under `background`, the fill otherwise — reaches
    shape_min_contrast (None: 8), at shape_connectivity (None: 8), with max(1, W * W // 5) <= n <= 3 * W * W pixels,
    W = ceil(target_width); the K largest (ties to the one that comes first in raster order; target 0 is the largest) give their
    centroids, rounded half to even, as guesses, and every guess is refined by the tracker's own detection on that frame, exactly
    like a given start location.  Animals near the walls are found, where the centre window sees none of them.  ValueError
    naming both numbers when fewer than K blobs are kept, for find="frame" without n_targets and for any other value.
    `exclusive` = True keeps the targets apart (this library's addition; include/pawsome_exclusive.h states the rule): the
    loop from the second selected frame on is BatchTracker.detect_chains_exclusive over all targets as one group — per step
    every target's window yields its best separated peaks and the targets share them out, so that no two take the same blob;
    a target that finds none of its own waits where it is.  `min_ratio` (None: 0.5) is the least share of a window's best
    response a second or later peak must reach to be taken, and `min_distance` (None: ceil(target_width)) the least distance
    between two peaks; at most 32 targets.  The result then gains a trailing `state`, int32 cuda [n_targets, m]: 0 for the
    bootstrap, the number of the pick a target was assigned (1: the functor's own answer), -1 where it was held.  Bootstrap,
    subpixel, diagnostic and n_targets work on the positions as before.  ValueError for min_ratio without exclusive.
    `motion` = True keeps the targets apart WITH A MOTION MODEL (this library's addition; include/pawsome_motion.h states the
    rule): the loop is BatchTracker.detect_chains_motion over all targets as one group — every target's window is centred on
    where its last uncontested displacement predicts it, the targets share out the peaks by nearness to their predictions,
    and a target whose window offers nothing above `min_response` (None: 0.0) coasts along its velocity for `coast` steps
    (None: 8) and then waits.  `min_distance` and `min_ratio` mean what they mean for `exclusive`, and the result gains the
    same trailing `state` (-1: held, the position is the prediction).  ValueError for motion together with exclusive, and for
    coast or min_response without motion or predict.
    `predict` = True gives every target an INDEPENDENT chain with the same motion model (this library's addition;
    include/pawsome_predict.h states the rule): the loop is BatchTracker.detect_chains_predicted, one launch for all targets
    where the plain loop is one launch — every target's window is centred on where its last displacement predicts it, and a
    target whose window offers nothing above `min_response` (None: 0.0) coasts for `coast` steps (None: 8) and then waits.
    Nothing keeps two targets apart.  The result gains the trailing `state`: 0 for the bootstrap, 1 assigned, -1 held.
    ValueError for predict together with motion or exclusive.
    `background` removes a STATIC BACKGROUND first (this library's addition; include/pawsome_background.h states the rule): an
    int K (1 ... 64) estimates the per-pixel lower median of background_samples(table, K) of the selected frames, a uint8 cuda
    tensor [h, w] is taken as the model itself (the empty arena).  The tracker then sees only the subtracted video,
    clamp(128 + frame - model, 0, 255): the fill is the mode of the first subtracted selected frame, the bootstrap (n_targets
    included) runs on that frame and the loop — plain, exclusive, motion or predict — on the subtracted frames, which exist at
    most `background_chunk` steps at a time in one reused buffer: chunk 0 starts from the bootstrap, every later chunk from the
    chunk before it (its last positions and, for motion and predict, its mstate), so the result does not depend on
    background_chunk.  subpixel measures on the subtracted frames; diagnostic draws on the original ones.  ValueError for
    background_chunk without background and for K outside 1 ... 64.
    `shape` = True measures HOW every target lies (this library's addition; include/pawsome_shape.h states the rule): the
    result gains `shape`, float64 cuda [n_targets, m, 6], as its LAST element, behind sub and state where those are present —
    BatchTracker.shapes at every returned position, held ones included, with `shape_radius` (None: ceil(target_width)) and
    `shape_min_contrast` (None: 8): (row, col) of the blob's centroid, theta, the major and minor axes and the equivalent
    width; NaN where no blob reaches the contrast.  It is measured on the frames the tracker saw: the subtracted ones under
    background, chunk by chunk as subpixel is, and independent of background_chunk.  headings(shape, indices) turns theta into a
    heading along the motion.  ValueError for shape_radius or shape_min_contrast without shape; every result without the
    keyword is what it is today.
    `shape_connectivity` = 4 or 8 measures `shape` over the CONNECTED BLOB under every position instead
    (BatchTracker.blobs; include/pawsome_blob.h states the rule): a second object inside the radius is left out.  None is the
    shape rule, bit for bit as before.  ValueError without shape.
    `shape_split` = True measures every target's blob INSIDE ITS NEAREST-CENTRE CELL among the step's positions of all targets,
    held ones included (BatchTracker.split_blobs; include/pawsome_split.h states the rule): two animals that touch are
    measured one by one, where shape_connectivity alone reports one merged body for both.  The result then gains `contact`,
    int32 cuda [n_targets, m], as its last element behind `shape`: the rule's n_contact, > 0 where the target's blob touches a
    neighbour's side.  One call without background, one per chunk under it, independent of background_chunk.  ValueError
    without shape=True and a shape_connectivity; with False every result is bit for bit what it is without the keyword."""
    import torch
    from ._args import background_k, device_frames, exclusive_args, motion_args, peaks_args, predict_args
    from .batch import BatchTracker, mode_device
    chunk = _check_sink(diagnostic, diagnostic_chunk)
    shape_kw = _shape_keywords(shape, shape_radius, shape_min_contrast, shape_connectivity)
    if not isinstance(shape_split, bool):
        raise TypeError("shape_split must be True or False")
    if shape_split and (shape_kw is None or shape_kw[2] is None):
        raise ValueError("shape_split belongs to shape=True with a shape_connectivity of 4 or 8")
    if isinstance(background_chunk, bool) or not isinstance(background_chunk, (int, np.integer)):
        raise TypeError("background_chunk must be an integer")
    if background_chunk < 1:
        raise ValueError(f"background_chunk: {background_chunk} is not a positive number of steps")
    if background is None:
        if background_chunk != 256:
            raise ValueError("background_chunk belongs to background")
    elif not isinstance(background, torch.Tensor):
        background = background_k(background, "background")
    if n_targets is not None:
        if start_locations is not None:
            raise ValueError("n_targets finds the targets itself: give it, or start_locations, not both")
        n_targets, md = peaks_args(n_targets, min_distance, "n_targets")
        start_locations = [None] * n_targets
    elif min_distance is not None and not exclusive and motion is not True:
        raise ValueError("min_distance belongs to n_targets and exclusive")
    if not isinstance(find, str) or find not in ("window", "frame"):
        raise ValueError(f'find: {find!r} is neither "window" nor "frame"')
    if find != "window" and n_targets is None:
        raise ValueError("find belongs to n_targets")
    if not isinstance(exclusive, bool):
        raise TypeError("exclusive must be True or False")
    if not isinstance(motion, bool):
        raise TypeError("motion must be True or False")
    if not isinstance(predict, bool):
        raise TypeError("predict must be True or False")
    if predict and (motion or exclusive):
        raise ValueError("predict walks independent chains, motion and exclusive joint ones: give one of predict, motion and exclusive")
    if motion and exclusive:
        raise ValueError("motion and exclusive are two rules for one loop: give one of them")
    if min_ratio is not None and not exclusive and not motion:
        raise ValueError("min_ratio belongs to exclusive")
    if (coast is not None or min_response is not None) and not motion and not predict:
        raise ValueError("coast and min_response belong to motion and predict")
    if predict:
        pred = predict_args(0.0 if min_response is None else min_response, 8 if coast is None else coast)
    if exclusive or motion:
        n_locs = len(start_locations) if isinstance(start_locations, list) else 1
        excl = exclusive_args(max(n_locs, 1), None, min_distance, 0.5 if min_ratio is None else min_ratio)
    if motion:
        excl = motion_args(max(n_locs, 1), None, min_distance, excl[2], 0.0 if min_response is None else min_response,
                           8 if coast is None else coast)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 3):
        raise TypeError("frames must be a uint8 cuda tensor [n_frames, h, w]")
    n, h, w = (int(v) for v in frames.shape)
    table = fps_table(rate, n, start, stop, fps)
    m = len(table)
    ts = time_axis(start, stop, fps, first=m)
    locs = list(start_locations) if isinstance(start_locations, list) else [start_locations]
    if not locs:
        raise ValueError("start_locations: an empty list names no target")
    nt = len(locs)
    if window_size is None:
        window_size = guess_window_size(target_width)            # :136
    window_size = fix_window_size(window_size)                   # :142
    dev = frames.device
    if isinstance(background, torch.Tensor):
        device_frames(background, "background", 2, (h, w), dev.index)
    bstep = int(background_chunk)

    def walk(bt, fr, tab, starts, first, mstate):
        """One call of the loop the keywords chose over the steps `tab` of the stack `fr`: (positions [nt, len(tab), 2], state
        or None, mstate or None)."""
        if exclusive:    # all targets as ONE group: excl is the rule's (k, min_distance, min_ratio[, min_response, coast])
            o, st = bt.detect_chains_exclusive(fr, tab[None, :], starts.unsqueeze(0).contiguous(), None, excl[1] or None, *excl[2:], first=first)
            return o[0], st[0], None
        if motion:
            o, st, ms = bt.detect_chains_motion(fr, tab[None, :], starts.unsqueeze(0).contiguous(), None, excl[1] or None, *excl[2:],
                                                first=first, mstate=mstate)
            return o[0], st[0], ms
        if predict:
            return bt.detect_chains_predicted(fr, np.tile(tab, (nt, 1)), starts, *pred, mstate=mstate, first=first)
        return bt.detect_chains_indexed(fr, np.tile(tab, (nt, 1)), starts, first=first), None, None

    with torch.cuda.device(dev):
        bg = buf = None
        seen, f0 = frames, int(table[0])          # the stack the tracker sees, and its first selected frame in it
        if background is not None:
            from .background import Background
            bg = Background(h, w, dev.index)
        bt = None
        try:
            if bg is not None:
                if isinstance(background, torch.Tensor):
                    bg.set(background)
                else:
                    from .background import background_samples
                    bg.estimate(frames, background_samples(table, background))
                buf = torch.empty((min(bstep, m), h, w), dtype=torch.uint8, device=dev)
                bg.subtract(frames, table[:len(buf)], out=buf)              # chunk 0: its first frame is the bootstrap frame
                seen, f0 = buf, 0
            fill = mode_device(seen[f0])                                 # :159, :47
            bt = BatchTracker(h, w, target_width, window_size, darker_target, fill, device=dev.index)
            # the first positions, :92-107: one functor application per target on the first selected frame
            guesses = torch.tensor([get_guess(loc, frames[0], sar) for loc in locs], dtype=torch.int32, device=dev).reshape(nt, 2)
            on_f0 = torch.full((nt,), f0, dtype=torch.int32, device=dev)
            starts = bt.detect(seen, guesses, on_f0)                                                      # :95
            auto = torch.tensor([loc is None for loc in locs], device=dev)
            if n_targets is not None and find == "frame":
                from .frame_blobs import FrameBlobs, frame_start_guesses
                W = int(np.ceil(target_width))
                with FrameBlobs(h, w, dev.index, steps_in_flight=1) as fb:
                    kw = dict(table=[f0], level=128 if bg is not None else int(fill), darker_target=bool(darker_target),
                              min_contrast=shape_kw[1] if shape_kw else 8, connectivity=(shape_kw[2] if shape_kw else None) or 8,
                              min_area=max(1, W * W // 5), max_area=3 * W * W)
                    count, words = fb.find(seen, cap=64, **kw)
                    kept = int(count[0, 0])
                    if kept > words.shape[1]:        # the list is cut: once more with room for all of them
                        count, words = fb.find(seen, cap=kept, **kw)
                    words = words[0, :kept].cpu().numpy()
                if kept < n_targets:
                    raise ValueError(f"n_targets = {n_targets}, but the first frame holds only {kept} blob(s) of "
                                     f"{kw['min_area']} ... {kw['max_area']} pixels")
                guesses = torch.tensor(frame_start_guesses(words, n_targets), dtype=torch.int32, device=dev).reshape(nt, 2)
                starts = bt.detect(seen, guesses, on_f0)
            elif n_targets is not None:
                bt4 = BatchTracker(h, w, target_width, (h // 4, w // 4), darker_target, fill, device=dev.index)   # :102-103
                try:
                    ij, peak, _ = bt4.detect_peaks(seen, guesses[:1], n_targets, md or None, on_f0[:1])           # :104, and K - 1 more
                    bt4.sync()
                finally:
                    bt4.close()
                found = int((peak[0] > 0).sum())         # (pick order is value order: the positive ones come first)
                if found < n_targets:
                    raise ValueError(f"n_targets = {n_targets}, but the bootstrap window holds only {found} separated peak(s) "
                                     "with a positive response")
                starts = ij[0].contiguous()
            elif bool(auto.any()):
                bt4 = BatchTracker(h, w, target_width, (h // 4, w // 4), darker_target, fill, device=dev.index)   # :102-103
                try:
                    starts = torch.where(auto[:, None], bt4.detect(seen, guesses, on_f0), starts).contiguous()    # :104
                    bt4.sync()           # a guess outside the padded frame raises here, like the reference's BoundsError
                finally:
                    bt4.close()
            # the loop from the second selected frame on, :161-167: every target over the same table
            sub = shp = contact = None

            def shapes_of(fr, o, fi):
                """`shape` [nt, steps, 6] at the positions o [nt, steps, 2] — and the contact counts [nt, steps] under shape_split."""
                if not shape_split:
                    return _shapes_or_blobs(bt, fr, o.reshape(-1, 2), fi, shape_kw).view(nt, -1, 6), None
                sh, words = bt.split_blobs(fr, o, fi.view(nt, -1), shape_kw[0] or None, shape_kw[1], shape_kw[2], targets_first=True, want_sums=True)
                return sh, words[:, :, 11]

            if bg is None:
                out, state, _ = walk(bt, frames, table, starts, 1, None)
                if subpixel or shape_kw:
                    fi = torch.from_numpy(np.tile(table, nt)).to(dev)
                if subpixel:
                    sub = bt.measure(frames, out.view(-1, 2), fi).view(nt, m, 2)
                if shape_kw:
                    shp, contact = shapes_of(frames, out, fi)
            else:                        # the same over the subtracted frames, a buffer of them at a time
                out = torch.zeros((nt, m, 2), dtype=torch.int32, device=dev)
                state = torch.zeros((nt, m), dtype=torch.int32, device=dev) if exclusive or motion or predict else None
                sub = torch.empty((nt, m, 2), dtype=torch.float64, device=dev) if subpixel else None
                shp = torch.empty((nt, m, 6), dtype=torch.float64, device=dev) if shape_kw else None
                contact = torch.empty((nt, m), dtype=torch.int32, device=dev) if shape_split else None
                mstate = None
                for k0 in range(0, m, bstep):
                    nk = min(bstep, m - k0)
                    if k0:
                        bg.subtract(frames, table[k0:k0 + nk], out=buf[:nk])     # (behind the last chunk's walk, in stream order)
                        starts = out[:, k0 - 1].contiguous()
                    o, st, mstate = walk(bt, buf[:nk], np.arange(nk, dtype=np.int32), starts, 0 if k0 else 1, mstate)
                    out[:, k0:k0 + nk] = o
                    if state is not None:
                        state[:, k0:k0 + nk] = st
                    if subpixel or shape_kw:
                        fi = torch.from_numpy(np.tile(np.arange(nk, dtype=np.int32), nt)).to(dev)
                    if subpixel:
                        sub[:, k0:k0 + nk] = bt.measure(buf[:nk], o.reshape(-1, 2).contiguous(), fi).view(nt, nk, 2)
                    if shape_kw:
                        shp[:, k0:k0 + nk], part = shapes_of(buf[:nk], o.contiguous(), fi)
                        if shape_split:
                            contact[:, k0:k0 + nk] = part
            bt.sync()                    # what the kernels raised (PdogError) surfaces before the positions are handed out
            if diagnostic is not None:
                from .diagnose import Diagnose
                with Diagnose(darker_target, dev.index) as dia:
                    dia.set_targets(nt)
                    _render_steps(dia, frames, table, out, chunk, diagnostic)
            res = (ts, out, sub) if subpixel else (ts, out)
            if exclusive or motion or predict:
                res += (state,)
            if shape_split:
                return res + (shp, contact.contiguous())
            return res + (shp,) if shape_kw else res
        finally:
            if bt is not None:
                bt.close()
            if bg is not None:
                bg.close()
