"""Device-resident batches and multi-GPU sharding for the DoG + argmax path.

`BatchTracker` is n independent applications of the reference functor
(/root/reference/src/PawsomeTracker.jl:55-62) on frames that already live in
HBM; torch is used only for device memory, streams and torch.distributed
(RCCL).  Sharding: contiguous window ranges per rank, no data-path
collective, one gather of the int32 (row, col) pairs to rank 0.
"""
import ctypes as C

from . import _lib
from ._args import blob_args, device_array, device_frames, exclusive_args, frame_index_ptr, host_i32, host_table, motion_args, peaks_args, predict_args, shape_args


def _targets_of(starts):
    """n_targets of a group walk's starts, [n_groups, n_targets, 2]; the rest of the shape is judged with the table's."""
    import torch
    if not isinstance(starts, torch.Tensor) or starts.dim() != 3:
        raise TypeError("starts must be an int32 cuda tensor [n_groups, n_targets, 2]")
    return int(starts.shape[1])


class BatchTracker(_lib.TrackerHandle):
    _clips = None

    def __init__(self, frame_h, frame_w, target_width, window_size, darker_target, fill, device=0):
        super().__init__(_lib.new_handle(_lib.lib().pdog_create, int(device), int(frame_h), int(frame_w), float(target_width),
                                         int(window_size[0]), int(window_size[1]), int(bool(darker_target)), int(fill)),
                         "pdog_destroy")
        self.device = int(device)
        self.frame_h, self.frame_w = int(frame_h), int(frame_w)
        self._hw = (self.frame_h, self.frame_w)

    def use_torch_stream(self):
        """Launch on torch's current stream.  Every detect* call does this: the kernels are asynchronous, and
        only work queued on the stream torch's caching allocator knows about is safe against a tensor
        (guesses, frames) being dropped by the caller and its memory reused before the kernels ran."""
        import torch
        _lib.check(_lib.lib().pdog_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def detect(self, frames, guesses, frame_index=None, out=None, want_resp=False):
        """frames: uint8 cuda tensor [nf, h, w] (row stride may exceed w); guesses: int32 cuda [n, 2]
        1-based (row, col).  Returns int32 cuda [n, 2] (and float32 [n, win_w, win_h] — each
        window column-major, i.e. resp[b].T is the h x w response — when want_resp)."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        n = device_array(guesses, "guesses", torch.int32, (None, 2)).shape[0]
        fi = frame_index_ptr(frame_index, n)
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int32, device=frames.device)
        resp = None
        if want_resp:
            info = self.info()
            resp = torch.empty((n, info.win_w, info.win_h), dtype=torch.float32, device=frames.device)
        _lib.check(_lib.lib().pdog_detect_batch(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(guesses.data_ptr()), n, C.c_void_p(out.data_ptr()),
            C.c_void_p(resp.data_ptr()) if want_resp else None))
        return (out, resp) if want_resp else out

    def detect_peaks(self, frames, guesses, k, min_distance=None, frame_index=None, want_resp=False):
        """The k best, mutually separated peaks of every window (pdog_detect_peaks; this library's addition, the rule is
        stated in include/pawsome_peaks.h): frames, guesses and frame_index as for detect.  Pick 1 is detect's position; picks
        2 ... k are the local maxima of the window's FP32 response inside the frame, taken greedily by value, none closer
        than min_distance pixels (None: ceil(target_width)) to an earlier pick.  Returns (ij int32 cuda [n, k, 2], peak
        float32 cuda [n, k], count int32 cuda [n]): count picks per window in pick order, the rest (0, 0) and -inf — and the
        maps, float32 [n, win_w, win_h] as detect hands them out, when want_resp.  Without want_resp the maps live in scratch
        of the tracker's (PDOG_MAP_MB) and large batches go in chunks."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        n = device_array(guesses, "guesses", torch.int32, (None, 2)).shape[0]
        fi = frame_index_ptr(frame_index, n)
        k, md = peaks_args(k, min_distance)
        ij = torch.empty((n, k, 2), dtype=torch.int32, device=frames.device)
        peak = torch.empty((n, k), dtype=torch.float32, device=frames.device)
        count = torch.empty((n,), dtype=torch.int32, device=frames.device)
        resp = None
        if want_resp:
            info = self.info()
            resp = torch.empty((n, info.win_w, info.win_h), dtype=torch.float32, device=frames.device)
        _lib.check(_lib.lib().pdog_detect_peaks(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(guesses.data_ptr()), n, k, md, C.c_void_p(ij.data_ptr()), C.c_void_p(peak.data_ptr()),
            C.c_void_p(count.data_ptr()), C.c_void_p(resp.data_ptr()) if want_resp else None))
        return (ij, peak, count, resp) if want_resp else (ij, peak, count)

    def detect_host(self, frames, guesses, frame_index=None):
        """The same n applications on frames in HOST memory (numpy uint8 [nf, h, w], the layout
        `read!(vid, trckr.img.data)`, src/PawsomeTracker.jl:166, produces): only the window tiles are uploaded,
        in chunks that overlap the kernels.  guesses int32 [n, 2]; returns numpy int32 [n, 2].  Synchronous."""
        import numpy as np
        self.use_torch_stream()
        if not isinstance(frames, np.ndarray) or frames.dtype != np.uint8 or frames.ndim != 3:
            raise TypeError("frames must be a numpy uint8 array [n, h, w]")
        if frames.strides[2] != 1 or frames.shape[1:] != self._hw:
            raise ValueError(f"frames: {frames.shape[1]} x {frames.shape[2]} with last stride {frames.strides[2]}, "
                             f"the tracker needs {self.frame_h} x {self.frame_w} with last stride 1")
        g = np.ascontiguousarray(guesses, np.int32)
        n = g.shape[0]
        if g.shape != (n, 2):
            raise ValueError(f"guesses: shape {g.shape}, expected (n, 2)")
        out = np.empty((n, 2), np.int32)
        fi_arr = host_i32(frame_index, "frame_index", n)
        _lib.check(_lib.lib().pdog_detect_batch_host(
            self._h, C.c_void_p(frames.ctypes.data), frames.strides[0], frames.strides[1], frames.shape[0],
            None if fi_arr is None else C.c_void_p(fi_arr.ctypes.data), C.c_void_p(g.ctypes.data), n, C.c_void_p(out.ctypes.data)))
        return out

    def detect_chain(self, frames, start_guess, out=None):
        """The serial chain of src/PawsomeTracker.jl:163-169 on device-resident frames."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        n = frames.shape[0]
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int32, device=frames.device)
        g = (C.c_int32 * 2)(int(start_guess[0]), int(start_guess[1]))
        _lib.check(_lib.lib().pdog_detect_chain(self._h, C.c_void_p(frames.data_ptr()), frames.stride(0),
                                                frames.stride(1), n, g, C.c_void_p(out.data_ptr())))
        return out

    def detect_chain_progress(self, frames, start_guess):
        """detect_chain whose positions land in host memory as the frames finish (pdog_detect_chain_progress): returns a
        ChainProgress to poll — what a per-frame consumer such as the reference's diagnostic overlay
        (src/diagnose.jl:30-38) needs from a device-side chain."""
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        cp = ChainProgress(self, frames.shape[0], frames)
        g = (C.c_int32 * 2)(int(start_guess[0]), int(start_guess[1]))
        try:
            _lib.check(_lib.lib().pdog_detect_chain_progress(self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                                             frames.shape[0], g, cp._out._h, cp._prog._h))
        except Exception:
            cp.close()      # nothing was queued: the pinned buffers go back at once
            raise
        return cp

    def detect_chains(self, frames, start_guesses, out=None):
        """Many clips at once (one persistent launch for l = 65): frames uint8 cuda [n_clips, n_frames, h, w],
        start_guesses int32 cuda [n_clips, 2]; returns int32 cuda [n_clips, n_frames, 2]."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 4, self._hw)
        nc, nf = frames.shape[0], frames.shape[1]
        device_array(start_guesses, "start_guesses", torch.int32, (nc, 2))
        if out is None:
            out = torch.empty((nc, nf, 2), dtype=torch.int32, device=frames.device)
        _lib.check(_lib.lib().pdog_detect_chains(self._h, C.c_void_p(frames.data_ptr()), frames.stride(1), frames.stride(2),
                                                 nf, nc, C.c_void_p(start_guesses.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def _table_walk(self, frames, frame_table, starts, first, n_targets=None, state=False, out=None, name="starts"):
        """What the methods over a frame table begin with: torch's stream, the table on the host, `first` (None: the library's
        to judge), the frame stack, starts int32 cuda [n_rows, 2] — [n_rows, n_targets, 2] with n_targets —, and the zeroed
        outputs: positions [n_rows, (n_targets,) n_steps, 2] (`out`, checked, where one is given) and, with `state`, the states
        beside them.  Returns (the library's arguments behind the handle: the stack, the table and its sizes; positions;
        states or None)."""
        import torch
        self.use_torch_stream()
        table = host_table(frame_table, "frame_table")
        nr, ns = table.shape
        if first is not None and (isinstance(first, bool) or first not in (0, 1)):
            raise ValueError(f"first: {first!r} is neither 0 nor 1")
        device_frames(frames, "frames", 3, self._hw)
        rows = (nr,) if n_targets is None else (nr, n_targets)
        device_array(starts, name, torch.int32, rows + (2,))
        if out is None:
            out = torch.zeros(rows + (ns, 2), dtype=torch.int32, device=frames.device)
        device_array(out, "out", torch.int32, rows + (ns, 2))
        st = torch.zeros(rows + (ns,), dtype=torch.int32, device=frames.device) if state else None
        tab = table.ctypes.data_as(C.c_void_p)      # (data_as keeps the array alive as long as the pointer)
        return (C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], tab, ns, nr), out, st

    def detect_chains_indexed(self, frames, frame_table, start_guesses, first=0, out=None):
        """Chains over a frame table (pdog_detect_chains_indexed): frames uint8 cuda [n_frames, h, w] is ONE stack that every
        clip shares; frame_table — rows of integers [n_clips, n_steps], host side — names the frame of each step, and a clip
        ends where its row turns negative; start_guesses int32 cuda [n_clips, 2].  first = 0: out[c][0] = functor(frame
        table[c][0], start[c]); first = 1: out[c][0] = start[c] as given and the loop starts at step 1
        (src/PawsomeTracker.jl:161-167).  Several rows may name the same frames (several targets in one video, several
        start/stop windows of it).  The library checks the table before it launches anything (PdogError, PDOG_E_ARG, for an
        entry >= n_frames or a non-negative entry behind a negative one).  Returns int32 cuda [n_clips, n_steps, 2]; rows at
        and beyond a clip's end are not written (a fresh `out` is zeroed)."""
        walk, out, _ = self._table_walk(frames, frame_table, start_guesses, None, out=out, name="start_guesses")
        _lib.check(_lib.lib().pdog_detect_chains_indexed(self._h, *walk, int(first), C.c_void_p(start_guesses.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def assign_exclusive(self, prev, ij, peak, count, min_distance=None, min_ratio=0.5):
        """The exclusive step alone (pdog_assign_exclusive; this library's addition, the rule is stated in
        include/pawsome_exclusive.h): per group the targets share out the peaks of their windows so that no two take the same
        blob.  prev int32 cuda [n_groups, n_targets, 2], the positions the windows were centred on; ij int32 cuda
        [n_groups, n_targets, k, 2], peak float32 cuda [n_groups, n_targets, k] and count int32 cuda [n_groups, n_targets]:
        what detect_peaks returned for the n_groups * n_targets windows, reshaped.  Returns (positions int32 cuda
        [n_groups, n_targets, 2], state int32 cuda [n_groups, n_targets]): state is the number of the pick a target was
        assigned, 1 ... k, or -1 where it found no blob of its own and is held at prev."""
        import torch
        self.use_torch_stream()
        if not isinstance(prev, torch.Tensor) or prev.dim() != 3 or not isinstance(ij, torch.Tensor) or ij.dim() != 4:
            raise TypeError("prev must be an int32 cuda tensor [n_groups, n_targets, 2], ij one [n_groups, n_targets, k, 2]")
        ng, nt, k = int(ij.shape[0]), int(ij.shape[1]), int(ij.shape[2])
        if ng < 1:
            raise ValueError("ij: no group")
        k, md, rho = exclusive_args(nt, k, min_distance, min_ratio)
        device_array(prev, "prev", torch.int32, (ng, nt, 2))
        device_array(ij, "ij", torch.int32, (ng, nt, k, 2))
        device_array(peak, "peak", torch.float32, (ng, nt, k))
        device_array(count, "count", torch.int32, (ng, nt))
        out = torch.empty((ng, nt, 2), dtype=torch.int32, device=ij.device)
        state = torch.empty((ng, nt), dtype=torch.int32, device=ij.device)
        _lib.check(_lib.lib().pdog_assign_exclusive(
            self._h, ng, nt, k, md, rho, C.c_void_p(prev.data_ptr()), C.c_void_p(ij.data_ptr()), C.c_void_p(peak.data_ptr()),
            C.c_void_p(count.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(state.data_ptr())))
        return out, state

    def detect_chains_exclusive(self, frames, frame_table, starts, k=None, min_distance=None, min_ratio=0.5, first=0):
        """The exclusive walk over a frame table (pdog_detect_chains_exclusive): frames uint8 cuda [n_frames, h, w] is one stack;
        frame_table [n_groups, n_steps], host side, names each step's frame for a GROUP — the targets of one video, which
        share its row — as for detect_chains_indexed; starts int32 cuda [n_groups, n_targets, 2].  Per step every target's
        window yields its k best peaks (k None: min(32, 2 * n_targets); min_distance None: ceil(target_width)) and the
        group's targets share them out as assign_exclusive states; first as for detect_chains_indexed (first = 1 files the
        starts as given, with state 0).  Returns (indices int32 cuda [n_groups, n_targets, n_steps, 2], state int32 cuda
        [n_groups, n_targets, n_steps]); steps at and beyond a group's end are not written (both are zeroed)."""
        nt = _targets_of(starts)
        k, md, rho = exclusive_args(nt, k, min_distance, min_ratio)
        walk, out, state = self._table_walk(frames, frame_table, starts, first, nt, state=True)
        _lib.check(_lib.lib().pdog_detect_chains_exclusive(self._h, *walk, nt, int(first), k, md, rho, C.c_void_p(starts.data_ptr()),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(state.data_ptr())))
        return out, state

    def assign_motion(self, prev, mstate, ij, peak, count, min_distance=None, min_ratio=0.5, min_response=0.0, coast=8):
        """The motion step alone (pdog_assign_motion; this library's addition, the rule is stated in include/pawsome_motion.h):
        every target takes the free peak NEAREST to its prediction clamp(p + v), a target that finds none coasts along it.
        prev int32 cuda [n_groups, n_targets, 2], the positions p; mstate int32 cuda [n_groups, n_targets, 4], (v_row, v_col,
        n_held, 0), UPDATED IN PLACE; ij, peak and count as for assign_exclusive — what detect_peaks returned for the windows
        at the PREDICTIONS.  An entry must exceed min_response and reach min_ratio times its window's best; a held target
        keeps its velocity for `coast` steps.  Returns (positions int32 cuda [n_groups, n_targets, 2], state int32 cuda
        [n_groups, n_targets], next guesses int32 cuda [n_groups, n_targets, 2]): state is the number of the pick a target was
        assigned, 1 ... k, or -1 where it was held and its position is the prediction."""
        import torch
        self.use_torch_stream()
        if not isinstance(prev, torch.Tensor) or prev.dim() != 3 or not isinstance(ij, torch.Tensor) or ij.dim() != 4:
            raise TypeError("prev must be an int32 cuda tensor [n_groups, n_targets, 2], ij one [n_groups, n_targets, k, 2]")
        ng, nt, k = int(ij.shape[0]), int(ij.shape[1]), int(ij.shape[2])
        if ng < 1:
            raise ValueError("ij: no group")
        k, md, rho, m, coast = motion_args(nt, k, min_distance, min_ratio, min_response, coast)
        device_array(prev, "prev", torch.int32, (ng, nt, 2))
        device_array(mstate, "mstate", torch.int32, (ng, nt, 4))
        device_array(ij, "ij", torch.int32, (ng, nt, k, 2))
        device_array(peak, "peak", torch.float32, (ng, nt, k))
        device_array(count, "count", torch.int32, (ng, nt))
        out = torch.empty((ng, nt, 2), dtype=torch.int32, device=ij.device)
        state = torch.empty((ng, nt), dtype=torch.int32, device=ij.device)
        nxt = torch.empty((ng, nt, 2), dtype=torch.int32, device=ij.device)
        P = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().pdog_assign_motion(self._h, ng, nt, k, md, rho, m, coast, P(prev), P(mstate), P(ij), P(peak), P(count),
                                                 P(out), P(state), P(nxt)))
        return out, state, nxt

    def detect_chains_motion(self, frames, frame_table, starts, k=None, min_distance=None, min_ratio=0.5, min_response=0.0, coast=8,
                             first=0, mstate=None):
        """The walk with a motion model over a frame table (pdog_detect_chains_motion): frames, frame_table, starts, k,
        min_distance, min_ratio and first as for detect_chains_exclusive.  Per step every target's window is centred on its
        prediction and the group's targets share out the peaks as assign_motion states.  mstate None: the walk starts at
        rest; otherwise int32 cuda [n_groups, n_targets, 4], the state a former call returned — it is updated in place, and
        a walk continued from a call's last positions and its mstate equals the one-call walk.  Returns (indices int32 cuda
        [n_groups, n_targets, n_steps, 2], state int32 cuda [n_groups, n_targets, n_steps], mstate); steps at and beyond a
        group's end are not written (both are zeroed)."""
        import torch
        nt = _targets_of(starts)
        k, md, rho, m, coast = motion_args(nt, k, min_distance, min_ratio, min_response, coast)
        walk, out, state = self._table_walk(frames, frame_table, starts, first, nt, state=True)
        if mstate is None:
            mstate = torch.zeros((state.shape[0], nt, 4), dtype=torch.int32, device=frames.device)
        device_array(mstate, "mstate", torch.int32, (state.shape[0], nt, 4))
        _lib.check(_lib.lib().pdog_detect_chains_motion(self._h, *walk, nt, int(first), k, md, rho, m, coast, C.c_void_p(starts.data_ptr()),
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(mstate.data_ptr())))
        return out, state, mstate

    def detect_chains_predicted(self, frames, frame_table, starts, min_response=0.0, coast=8, mstate=None, first=0):
        """Independent chains with a motion model over a frame table, in one launch where detect_chains_indexed is one launch
        (pdog_detect_chains_predicted; this library's addition, the rule is stated in include/pawsome_predict.h): frames,
        frame_table, starts int32 cuda [n_clips, 2] and first as for detect_chains_indexed.  Per step a clip's window is
        centred on its prediction clamp(p + v); a window whose FP32 maximum does not exceed min_response HOLDS the clip, which
        then coasts along v for `coast` steps and waits.  mstate None: every clip starts at rest; otherwise int32 cuda
        [n_clips, 4], (v_row, v_col, n_held, 0), the state a former call returned — it is updated in place, and a walk continued
        from a call's last positions and its mstate equals the one-call walk.  Returns (indices int32 cuda [n_clips, n_steps, 2],
        state int32 cuda [n_clips, n_steps] — 1 assigned, -1 held, 0 the start filed by first = 1 —, mstate); steps at and beyond
        a clip's end are not written (both are zeroed)."""
        import torch
        m, coast = predict_args(min_response, coast)
        walk, out, state = self._table_walk(frames, frame_table, starts, first, state=True)
        if mstate is None:
            mstate = torch.zeros((state.shape[0], 4), dtype=torch.int32, device=frames.device)
        device_array(mstate, "mstate", torch.int32, (state.shape[0], 4))
        _lib.check(_lib.lib().pdog_detect_chains_predicted(self._h, *walk, int(first), m, coast, C.c_void_p(starts.data_ptr()),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(mstate.data_ptr())))
        return out, state, mstate

    def measure(self, frames, ij, frame_index=None, want_resp=False):
        """Sub-pixel positions (and peak responses) at tracked points (pdog_measure).  frames: uint8 cuda tensor
        [nf, h, w] (row stride may exceed w); ij: int32 cuda [n, 2], 1-based (row, col) — what detect / detect_chain
        returned; position b looks at frame frame_index[b] (int32 cuda [n]; None: frame b).  Returns float64 cuda [n, 2],
        1-based (row, col) — and float64 [n, 5], the response {c, up, down, left, right} at the position and its four
        neighbours, when want_resp: resp[:, 0] is the value `findmax` (src/PawsomeTracker.jl:59) drops.  Runs on torch's
        current stream like every detect*: behind a detect call it needs no synchronisation in between.  For the
        positions of detect_chains (frames [n_clips, n_frames, h, w], out [n_clips, n_frames, 2]):

            sub = bt.measure(frames.flatten(0, 1), out.view(-1, 2)).view(n_clips, n_frames, 2)
        """
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        n = device_array(ij, "ij", torch.int32, (None, 2)).shape[0]
        fi = frame_index_ptr(frame_index, n)
        sub = torch.empty((n, 2), dtype=torch.float64, device=frames.device)
        resp = torch.empty((n, 5), dtype=torch.float64, device=frames.device) if want_resp else None
        _lib.check(_lib.lib().pdog_measure(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(ij.data_ptr()), n, C.c_void_p(resp.data_ptr()) if want_resp else None,
            C.c_void_p(sub.data_ptr())))
        return (sub, resp) if want_resp else sub

    def shapes(self, frames, ij, frame_index=None, radius=None, min_contrast=8, want_sums=False):
        """How the target lies at tracked points (pdog_shape; this library's addition, the rule is stated in
        include/pawsome_shape.h): frames, ij and frame_index as for measure.  Around every position the pixels within `radius`
        (None: ceil(target_width), at most 127; otherwise 2 ... 127) that reach half the target's own contrast against the
        patch's median form a mask — empty where that contrast stays below min_contrast (1 ... 255) — and the mask's moments
        give the result, float64 cuda [n, 6]: (row, col) of its centroid, theta — the major axis, from +col towards +row, in
        (-pi/2, pi/2] —, the full major and minor axes, and width, the equivalent diameter (the number to use as
        target_width); all NaN for an empty mask.  With want_sums (shape, sums): sums int32 cuda [n, 8], the rule's integers
        (n, Sy, Sx, Syy, Syx, Sxx, b, c).  Runs on torch's current stream like every detect*: behind a detect call it needs
        no synchronisation in between."""
        import torch
        self.use_torch_stream()
        radius, min_contrast = shape_args(radius, min_contrast)
        device_frames(frames, "frames", 3, self._hw)
        n = device_array(ij, "ij", torch.int32, (None, 2)).shape[0]
        fi = frame_index_ptr(frame_index, n)
        shape = torch.empty((n, 6), dtype=torch.float64, device=frames.device)
        sums = torch.empty((n, 8), dtype=torch.int32, device=frames.device) if want_sums else None
        if n == 0:              # (an empty tensor has no address to hand over)
            return (shape, sums) if want_sums else shape
        _lib.check(_lib.lib().pdog_shape(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(ij.data_ptr()), n, radius, min_contrast, C.c_void_p(sums.data_ptr()) if want_sums else None,
            C.c_void_p(shape.data_ptr())))
        return (shape, sums) if want_sums else shape

    def blobs(self, frames, ij, frame_index=None, radius=None, min_contrast=8, connectivity=8, want_sums=False):
        """shapes() with the mask restricted to the CONNECTED BLOB under every position (pdog_blob; the rule is stated in
        include/pawsome_blob.h): of the mask only the component that holds the darkest (brightest) pixel of the 3 x 3 under the
        position is measured, pixels being neighbours across an edge (`connectivity` 4) or an edge or a corner (8).  A second
        object inside the patch is then left out; two objects that touch are still one blob.  Returns float64 cuda [n, 6] as
        shapes() does.  With want_sums (shape, sums): sums int32 cuda [n, 10], (n, Sy, Sx, Syy, Syx, Sxx, b, c, n_mask, n_rim):
        the first eight are shapes()'s integers over the blob — shape_derive(sums[..., :8], ij) gives the floats —, n_mask
        is the whole mask's pixel count (n_mask > n: something else in the patch reaches half the target's contrast) and
        n_rim counts the blob pixels on the patch's rim (n_rim > 0: the blob is cut by the radius)."""
        import torch
        self.use_torch_stream()
        radius, min_contrast, connectivity = blob_args(radius, min_contrast, connectivity)
        device_frames(frames, "frames", 3, self._hw)
        n = device_array(ij, "ij", torch.int32, (None, 2)).shape[0]
        fi = frame_index_ptr(frame_index, n)
        shape = torch.empty((n, 6), dtype=torch.float64, device=frames.device)
        sums = torch.empty((n, 10), dtype=torch.int32, device=frames.device) if want_sums else None
        if n == 0:              # (an empty tensor has no address to hand over)
            return (shape, sums) if want_sums else shape
        _lib.check(_lib.lib().pdog_blob(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(ij.data_ptr()), n, radius, min_contrast, connectivity,
            C.c_void_p(sums.data_ptr()) if want_sums else None, C.c_void_p(shape.data_ptr())))
        return (shape, sums) if want_sums else shape

    def split_blobs(self, frames, ij, frame_index=None, radius=None, min_contrast=8, connectivity=8, targets_first=False, want_sums=False):
        """blobs() for targets that may TOUCH (pdog_blob_split; the rule is stated in include/pawsome_split.h): positions come in
        sets, the n_targets (1 ... 32) targets of one frame, and every target's blob is grown only inside its nearest-centre cell
        — the pixels nearer to its own position than to any other position of its set (ties to the lower index) —, so two
        animals in contact are measured one by one.  ij int32 cuda contiguous [n_sets, n_targets, 2], or [n_targets, n_sets, 2]
        with targets_first (the layout of the chains' results); frame_index None (set s looks at frame s) or int32 cuda over the
        same two leading dimensions.  Returns float64 cuda [..., ..., 6] as blobs() does, in ij's layout.  With want_sums
        (shape, sums): sums int32 cuda [..., ..., 12], blobs()'s ten over the split blob (b, c and n_mask unchanged) and n_cell,
        the mask pixels inside the cell, and n_contact, the blob pixels with an edge neighbour in the mask outside the cell
        (n_contact > 0: the target touches a neighbour's side).  Alone in its set, or with every other target farther than 2 *
        radius away, a target gets blobs()'s ten integers bit for bit."""
        import torch
        self.use_torch_stream()
        radius, min_contrast, connectivity = blob_args(radius, min_contrast, connectivity)
        if not isinstance(targets_first, bool):
            raise TypeError("targets_first must be True or False")
        device_frames(frames, "frames", 3, self._hw)
        device_array(ij, "ij", torch.int32, (None, None, 2))
        d0, d1 = int(ij.shape[0]), int(ij.shape[1])
        n_sets, n_targets = (d1, d0) if targets_first else (d0, d1)
        if not 1 <= n_targets <= 32:
            raise ValueError(f"ij: {n_targets} targets per set, 1 ... 32 expected")
        fi = None if frame_index is None else device_array(frame_index, "frame_index", torch.int32, (d0, d1)).data_ptr()
        if fi is None and n_sets > frames.shape[0]:
            raise ValueError(f"ij: {n_sets} sets, but {frames.shape[0]} frames and no frame_index")
        shape = torch.empty((d0, d1, 6), dtype=torch.float64, device=frames.device)
        sums = torch.empty((d0, d1, 12), dtype=torch.int32, device=frames.device) if want_sums else None
        if n_sets == 0:         # (an empty tensor has no address to hand over)
            return (shape, sums) if want_sums else shape
        strides = (1, n_sets) if targets_first else (n_targets, 1)
        _lib.check(_lib.lib().pdog_blob_split(
            self._h, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1), frames.shape[0], fi,
            C.c_void_p(ij.data_ptr()), n_sets, n_targets, *strides, radius, min_contrast, connectivity,
            C.c_void_p(sums.data_ptr()) if want_sums else None, C.c_void_p(shape.data_ptr())))
        return (shape, sums) if want_sums else shape

    def _clips_handle(self):
        """The pdog_clips handle behind clip_modes / track_clips: created on first use, closed with the tracker."""
        if self._clips is None:
            self._clips = _lib.Handle(_lib.new_handle(_lib.lib().pdog_clips_create, self._h), "pdog_clips_destroy")
        return self._clips._h

    def clips_counters(self):
        """(mode calls with one workgroup per frame, mode calls with several, per-frame batches of track_clips, track_clips
        calls that took the detect_chains fast path) since the handle was created — pdog_clips_get_counters."""
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().pdog_clips_get_counters(self._clips_handle(), out))
        return tuple(int(v) for v in out)

    def set_clips_tuning(self, key, value=1):
        """pdog_clips_set_tuning: tests and A/B only."""
        _lib.check(_lib.lib().pdog_clips_set_tuning(self._clips_handle(), key.encode(), int(value)))

    def clip_modes(self, frames, frame_index=None, out=None):
        """mode(_img) (src/PawsomeTracker.jl:47) of many device-resident frames in one call (pdog_clips_modes): frames
        uint8 cuda [nf, h, w] (row stride may exceed w); entry b looks at frame frame_index[b] (int32 cuda [n]; None:
        every frame in order).  Returns an int32 cuda tensor [n]; nothing is read back."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 3, self._hw)
        fi = frame_index_ptr(frame_index, None)
        n = frames.shape[0] if fi is None else frame_index.shape[0]
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=frames.device)
        device_array(out, "out", torch.int32, (n,))
        _lib.check(_lib.lib().pdog_clips_modes(self._clips_handle(), C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                               frames.shape[0], fi, n, C.c_void_p(out.data_ptr())))
        return out

    def track_clips(self, frames, starts, fills=None, lengths=None, first=0, out=None):
        """Many clips, each with its own fill, length and start (pdog_clips_track): frames uint8 cuda
        [n_clips, n_frames, h, w] stacked as detect_chains requires, starts int32 cuda [n_clips, 2].  fills (None: the
        tracker's fill for all) and lengths (None: n_frames each) hold one value per clip — sequences, numpy arrays or
        tensors, brought to host int32.  first = 0: out[c][0] = functor(frame 0, starts[c]); first = 1: out[c][0] =
        starts[c] as given and the loop starts at frame 1 (src/PawsomeTracker.jl:161-167).  Returns int32 cuda
        [n_clips, n_frames, 2]; rows at and beyond a clip's length are not written (a fresh `out` is zeroed)."""
        import torch
        self.use_torch_stream()
        device_frames(frames, "frames", 4, self._hw)
        nc, nf = frames.shape[0], frames.shape[1]
        device_array(starts, "starts", torch.int32, (nc, 2))
        fa, la = host_i32(fills, "fills", nc), host_i32(lengths, "lengths", nc)
        if out is None:
            out = torch.zeros((nc, nf, 2), dtype=torch.int32, device=frames.device)
        device_array(out, "out", torch.int32, (nc, nf, 2))
        _lib.check(_lib.lib().pdog_clips_track(self._clips_handle(), C.c_void_p(frames.data_ptr()), frames.stride(1), frames.stride(2),
                                               nf, nc, None if fa is None else C.c_void_p(fa.ctypes.data),
                                               None if la is None else C.c_void_p(la.ctypes.data), int(first),
                                               C.c_void_p(starts.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def track_clips_indexed(self, frames, frame_table, starts, fills=None, first=0, out=None):
        """track_clips over a frame table (pdog_clips_track_indexed): frames uint8 cuda [n_frames, h, w] is one stack that the
        clips share, frame_table [n_clips, n_steps] names each step's frame as for detect_chains_indexed (a clip ends where
        its row turns negative: the lengths are the table's), fills holds one value per clip (None: the tracker's fill for
        all).  Returns int32 cuda [n_clips, n_steps, 2]; rows at and beyond a clip's end are not written (a fresh `out` is
        zeroed)."""
        walk, out, _ = self._table_walk(frames, frame_table, starts, None, out=out)
        fa = host_i32(fills, "fills", out.shape[0])
        _lib.check(_lib.lib().pdog_clips_track_indexed(self._clips_handle(), *walk, None if fa is None else C.c_void_p(fa.ctypes.data), int(first),
                                                       C.c_void_p(starts.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def close(self):
        if self._clips is not None:
            self._clips.close()          # before the tracker it borrows
            self._clips = None
        super().close()


class ChainProgress:
    """Host-visible state of a running chain: `done()` frames are finished and `positions[:done()]` are final
    (the library publishes the count with release order; numpy reads the pinned words afresh on every access)."""

    def __init__(self, bt, n_frames, keepalive=None):
        import numpy as np
        self._bt, self.n_frames, self._keepalive = bt, int(n_frames), keepalive
        alloc = _lib.lib().pdog_alloc_host
        out = _lib.Handle(_lib.new_handle(alloc, 8 * self.n_frames), "pdog_free_host")
        prog = _lib.Handle(_lib.new_handle(alloc, 4), "pdog_free_host")     # (should this raise, `out` frees itself)
        self._out, self._prog = out, prog
        self.positions = np.ctypeslib.as_array(C.cast(self._out._h, C.POINTER(C.c_int32)), shape=(self.n_frames, 2))
        self._done = np.ctypeslib.as_array(C.cast(self._prog._h, C.POINTER(C.c_int32)), shape=(1,))

    def done(self):
        return int(self._done[0])

    def wait(self):
        self._bt.sync()
        return self.positions.copy()

    def close(self):
        """Give the pinned buffers back.  The chain that writes them must have finished: the tracker's stream is
        drained first — unless the tracker itself is already closed (pdog_destroy drains its stream)."""
        if self._out._h is None:
            return
        try:
            if self._bt._h:
                self._bt.sync()          # may raise what the chain's kernels raised: the buffers go back regardless
        finally:
            self.positions = self._done = None
            self._out.close()
            self._prog.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupTracker(_lib.Handle):
    """Several GPUs of one node behind one handle (pdog_group_*): contiguous window shards per device, frames and
    guesses resident on the owning device, one RCCL gather of the int32 positions to the root device per batch
    (the sharded unit is the functor src/PawsomeTracker.jl:55-62, the gathered result :173).
    One host process drives every device; torch only provides the device memory."""

    def __init__(self, devices, frame_h, frame_w, target_width, window_size, darker_target, fill):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        super().__init__(_lib.new_handle(_lib.lib().pdog_group_create, len(self.devices), arr, int(frame_h), int(frame_w),
                                         float(target_width), int(window_size[0]), int(window_size[1]),
                                         int(bool(darker_target)), int(fill)), "pdog_group_destroy")
        self.frame_h, self.frame_w = int(frame_h), int(frame_w)

    @classmethod
    def local(cls, n_ranks, frame_h, frame_w, target_width, window_size, darker_target, fill, device=0):
        """Tests: a group of n_ranks trackers that all live on `device`, each with its own stream, whose gather is the
        library's stream-ordered stand-in instead of RCCL (pdog_group_test_create_local).  Everything else is the same code."""
        self = cls.__new__(cls)
        self.devices = [int(device)] * int(n_ranks)
        _lib.Handle.__init__(self, _lib.new_handle(_lib.lib().pdog_group_test_create_local, int(n_ranks), int(device), int(frame_h),
                                                   int(frame_w), float(target_width), int(window_size[0]), int(window_size[1]),
                                                   int(bool(darker_target)), int(fill)), "pdog_group_destroy")
        self.frame_h, self.frame_w = int(frame_h), int(frame_w)
        return self

    def size(self):
        return _lib.lib().pdog_group_size(self._h)

    def shard(self, n_total, rank):
        lo, hi = C.c_int(), C.c_int()
        _lib.check(_lib.lib().pdog_group_shard(self._h, int(n_total), int(rank), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def _tracker(self, rank):
        """Rank's tracker, borrowed: the group owns it."""
        return _lib.TrackerHandle(_lib.new_handle(_lib.lib().pdog_group_tracker, self._h, int(rank)), None)

    def info(self, rank=0):
        return self._tracker(rank).info()

    def stream(self, rank):
        """The hipStream_t (as an int) rank's tracker launches on."""
        return _lib.new_handle(_lib.lib().pdog_get_stream, self._tracker(rank)._h).value or 0

    def kernel_for_batch(self, n_per_rank, rank=0):
        return self._tracker(rank).kernel_for_batch(n_per_rank)

    def reserve(self, n_total):
        for r in range(len(self.devices)):
            lo, hi = self.shard(n_total, r)
            self._tracker(r).reserve(max(1, hi - lo))

    def detect(self, frames, guesses, n_total, out, frame_index=None):
        """frames[r]: uint8 cuda tensor [nf_r, h, w] on device r (same strides on every rank); guesses[r]: int32 cuda
        [n_r, 2] on device r, n_r = the size of rank r's shard of n_total; out: int32 cuda [n_total, 2] on the root
        device.  Asynchronous (each rank's tracker stream); sync() waits.  The caller keeps the tensors alive until then."""
        import torch
        nd = len(self.devices)
        if len(frames) != nd or len(guesses) != nd or (frame_index is not None and len(frame_index) != nd):
            raise ValueError(f"frames, guesses and frame_index hold one entry per device ({nd})")
        fi = None if frame_index is None else [None] * nd
        for r, dev in enumerate(self.devices):
            lo, hi = self.shard(n_total, r)
            f = device_frames(frames[r], f"frames[{r}]", 3, (self.frame_h, self.frame_w), dev)
            if f.stride(0) != frames[0].stride(0) or f.stride(1) != frames[0].stride(1):
                raise ValueError(f"frames[{r}]: every rank's frames must have the strides of frames[0]")
            device_array(guesses[r], f"guesses[{r}]", torch.int32, (hi - lo, 2), dev)
            if fi is not None and frame_index[r] is not None:
                fi[r] = device_array(frame_index[r], f"frame_index[{r}]", torch.int32, (hi - lo,), dev).data_ptr()
        device_array(out, "out", torch.int32, (n_total, 2), self.devices[0])
        P = C.c_void_p * nd
        fr = P(*[f.data_ptr() for f in frames])
        gs = P(*[q.data_ptr() for q in guesses])
        nf = (C.c_int * nd)(*[f.shape[0] for f in frames])
        _lib.check(_lib.lib().pdog_group_detect_batch(self._h, fr, frames[0].stride(0), frames[0].stride(1), nf,
                                                      None if fi is None else P(*fi), gs, int(n_total), C.c_void_p(out.data_ptr())))
        return out

    def sync(self):
        _lib.check(_lib.lib().pdog_group_sync(self._h))


def mode_device(frame):
    """mode(_img) (src/PawsomeTracker.jl:47, StatsBase tie rule) of a uint8 cuda tensor [h, w]."""
    import torch
    device_frames(frame, "frame", 2)
    out = C.c_int()
    dev = frame.device.index if frame.device.index is not None else torch.cuda.current_device()
    _lib.check(_lib.lib().pdog_mode_u8_device(dev, C.c_void_p(frame.data_ptr()), frame.shape[0], frame.shape[1], frame.stride(0),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(out)))
    return out.value


def shard_range(n, rank, world_size):
    """Contiguous window range [lo, hi) owned by `rank`: sizes differ by at most 1."""
    base, rem = divmod(int(n), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class _PendingGather:
    """Handle of an asynchronous gather_positions: wait() returns what the blocking call returns."""

    def __init__(self, work, bufs, sizes, is_dst):
        self._work, self._bufs, self._sizes, self._is_dst = work, bufs, sizes, is_dst

    def wait(self):
        import torch
        self._work.wait()
        if not self._is_dst:
            return None
        return torch.cat([self._bufs[r][: hi - lo] for r, (lo, hi) in enumerate(self._sizes)], 0)


def gather_positions(local_ij, n_total, group=None, dst=0, async_op=False):
    """Gather the per-rank int32 [n_local, 2] results to rank `dst` in shard order.
    The only collective on the path: 8 B per window (RCCL gather over xGMI with the
    nccl backend; gloo on CPU for tests).  Returns the [n_total, 2] tensor on dst, None elsewhere.
    With async_op=True the collective is only enqueued (it runs beside the next batch's kernels) and a
    handle is returned whose wait() gives that result."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    sizes = [shard_range(n_total, r, world) for r in range(world)]
    max_n = max(hi - lo for lo, hi in sizes)
    if local_ij.is_cuda and dist.get_backend(group) == "gloo":
        local_ij = local_ij.cpu()      # gloo has no device-memory gather: rehearsals and CPU tests go through host memory
    pad = torch.zeros((max_n, 2), dtype=torch.int32, device=local_ij.device)
    pad[: local_ij.shape[0]] = local_ij
    bufs = [torch.empty_like(pad) for _ in range(world)] if rank == dst else None
    work = dist.gather(pad, bufs, dst=dst, group=group, async_op=True)
    pending = _PendingGather(work, bufs, sizes, rank == dst)
    return pending if async_op else pending.wait()
