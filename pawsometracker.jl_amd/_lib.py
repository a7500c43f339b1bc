"""ctypes binding of include/pawsome_dog.h (the C-ABI drop-in boundary).

The HIP extension is the product path: if libpawsome_dog.so is missing this
module raises — there is no CPU fallback and nothing here touches oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PAWSOME_DOG_LIB selects another build of the same library (tuning builds with ablation variants)
LIB_PATH = os.environ.get("PAWSOME_DOG_LIB") or os.path.join(_HERE, "libpawsome_dog.so")

PDOG_OK, PDOG_E_ARG, PDOG_E_HIP, PDOG_E_NODEV, PDOG_E_RANGE, PDOG_E_ALLOC = range(6)
PDOG_MAX_ROW_STRIDE = 1 << 21   # include/pawsome_dog.h: the largest row stride an entry point accepts

class PdogInfo(C.Structure):
    _fields_ = [
        ("frame_h", C.c_int32), ("frame_w", C.c_int32),
        ("radius_h", C.c_int32), ("radius_w", C.c_int32),
        ("win_h", C.c_int32), ("win_w", C.c_int32),
        ("kernel_len", C.c_int32), ("fill", C.c_int32), ("darker_target", C.c_int32),
        ("n_strips", C.c_int32), ("strip_w", C.c_int32), ("variant", C.c_int32),
        ("sigma", C.c_double), ("target_width", C.c_double),
        ("algorithmic_bytes_per_window", C.c_int64), ("algorithmic_fma_per_window", C.c_int64),
    ]


_i, _d, _p, _i64, _s = C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_char_p
_pi, _pp, _pu64 = C.POINTER(_i), C.POINTER(_p), C.POINTER(C.c_uint64)

# every function include/pawsome_dog.h declares, in header order: name -> (restype, argtypes).  tests/test_abi_cpu.py
# holds this table against the header's prototypes and the library's exports.
PROTOTYPES = {
    "pdog_abi_version": (_i, []),
    "pdog_last_error": (_s, []),
    "pdog_sigma": (_d, [_d]),
    "pdog_default_window": (_i, [_d]),
    "pdog_kernel_len": (_i, [_d]),
    "pdog_gaussian_taps": (_i, [_d, _i, _p, _i]),
    "pdog_dense_kernel": (_i, [_d, _i, _p, _i]),
    "pdog_mode_u8": (_i, [_p, _i, _i, _i64, _pi]),
    "pdog_mode_u8_device": (_i, [_i, _p, _i, _i, _i64, _p, _pi]),
    "pdog_create": (_i, [_i, _i, _i, _d, _i, _i, _i, _i, _pp]),
    "pdog_destroy": (_i, [_p]),
    "pdog_get_info": (_i, [_p, C.POINTER(PdogInfo)]),
    "pdog_set_fill": (_i, [_p, _i]),
    "pdog_set_stream": (_i, [_p, _p]),
    "pdog_get_stream": (_i, [_p, _pp]),
    "pdog_reserve": (_i, [_p, _i]),
    "pdog_kernel_for_batch": (_i, [_p, _i, _pi]),
    "pdog_set_variant": (_i, [_p, _i]),
    "pdog_sync": (_i, [_p]),
    "pdog_set_exact": (_i, [_p, _i]),
    "pdog_set_tuning": (_i, [_p, _s, _i]),
    "pdog_get_exact": (_i, [_p, _pi, C.POINTER(_d), _pu64]),
    "pdog_get_exact_detail": (_i, [_p, _pu64]),
    "pdog_detect_batch": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _p, _p]),
    "pdog_subpixel": (_i, [_p, _p, _p]),
    "pdog_measure": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _p, _p]),
    "pdog_detect_host": (_i, [_p, _p, _i64, _p, _p, _p]),
    "pdog_window_tile": (_i, [_p, _i, _i, _i64, _i, _d, _i, _i, _p, _p, _i64]),
    "pdog_detect_batch_host": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _p]),
    "pdog_detect_chain": (_i, [_p, _p, _i64, _i64, _i, _p, _p]),
    "pdog_detect_chains": (_i, [_p, _p, _i64, _i64, _i, _i, _p, _p]),
    "pdog_clips_create": (_i, [_p, _pp]),
    "pdog_clips_destroy": (_i, [_p]),
    "pdog_clips_modes": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _p]),
    "pdog_clips_plan": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _pi]),
    "pdog_clips_track": (_i, [_p, _p, _i64, _i64, _i, _i, _p, _p, _i, _p, _p]),
    "pdog_clips_get_counters": (_i, [_p, _pu64]),
    "pdog_clips_set_tuning": (_i, [_p, _s, _i]),
    "pdog_alloc_host": (_i, [C.c_size_t, _pp]),
    "pdog_free_host": (_i, [_p]),
    "pdog_detect_chain_progress": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _p]),
    "pdog_group_create": (_i, [_i, _p, _i, _i, _d, _i, _i, _i, _i, _pp]),
    "pdog_group_destroy": (_i, [_p]),
    "pdog_group_size": (_i, [_p]),
    "pdog_group_tracker": (_i, [_p, _i, _pp]),
    "pdog_group_shard": (_i, [_p, _i, _i, _pi, _pi]),
    "pdog_shard_range": (_i, [_i, _i, _i, _pi, _pi]),
    "pdog_shard_owner": (_i, [_i, _i, _i, _pi, _pi]),
    "pdog_group_detect_batch": (_i, [_p, _p, _i64, _i64, _p, _p, _p, _i, _p]),
    "pdog_group_sync": (_i, [_p]),
    "pdog_group_test_compact": (_i, [_p, _i, _i, _p]),
    "pdog_group_test_create_local": (_i, [_i, _i, _i, _i, _d, _i, _i, _i, _i, _pp]),
    "pdog_diag_create": (_i, [_i, _i, _pp]),
    "pdog_diag_destroy": (_i, [_p]),
    "pdog_diag_point": (_i, [_i, _i, _p, _p]),
    "pdog_diag_render": (_i, [_p, _p, _p, _i64, _i64, _i, _i, _i, _p, _p]),
}
SYMBOLS = tuple(PROTOTYPES)

# the same for include/pawsome_video.h, which pawsome_dog.h includes: chains over a frame table (tests/test_video_cpu.py
# holds this table against that header)
VIDEO_PROTOTYPES = {
    "pdog_time_axis": (_i, [_d, _d, _d, _p, _i, _pi]),
    "pdog_fps_table": (_i, [_d, _i, _d, _d, _d, _p, _i, _pi]),
    "pdog_detect_chains_indexed": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _i, _i, _p, _p]),
    "pdog_clips_track_indexed": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _i, _p, _i, _p, _p]),
}
VIDEO_SYMBOLS = tuple(VIDEO_PROTOTYPES)

# the same for include/pawsome_prune.h, which pawsome_dog.h includes too: kept ranges of the roll batch path
# (tests/test_prune_cpu.py holds this table against that header)
PRUNE_PROTOTYPES = {
    "pdog_get_prune_counts": (_i, [_p, _pu64]),
    "pdog_get_batch_maxima": (_i, [_p, _i, _p]),
}
PRUNE_SYMBOLS = tuple(PRUNE_PROTOTYPES)

# the same for include/pawsome_overlay.h, the third header pawsome_dog.h includes: the overlay over a frame table and for
# several targets (tests/test_overlay_cpu.py holds this table against that header)
OVERLAY_PROTOTYPES = {
    "pdog_diag_set_targets": (_i, [_p, _i]),
    "pdog_diag_get_targets": (_i, [_p, _pi]),
    "pdog_diag_render_indexed": (_i, [_p, _p, _p, _i64, _i64, _i, _i, _i, _p, _i, _p, _i64, _i, _p]),
}
OVERLAY_SYMBOLS = tuple(OVERLAY_PROTOTYPES)
DIAG_MAX_TARGETS = 1024      # PDOG_DIAG_MAX_TARGETS

# the same for include/pawsome_peaks.h, a header of its own that includes pawsome_dog.h: the K best separated peaks of a
# window (tests/test_peaks_cpu.py holds this table against that header)
PEAKS_PROTOTYPES = {
    "pdog_detect_peaks": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "pdog_get_peaks_counts": (_i, [_p, _pu64]),
}
PEAKS_SYMBOLS = tuple(PEAKS_PROTOTYPES)
PEAKS_MAX_K = 32             # PDOG_PEAKS_MAX_K

# the same for include/pawsome_exclusive.h, which includes pawsome_peaks.h: several targets of one video kept apart
# (tests/test_exclusive_cpu.py holds this table against that header)
EXCLUSIVE_PROTOTYPES = {
    "pdog_assign_exclusive": (_i, [_p, _i, _i, _i, _i, _d, _p, _p, _p, _p, _p, _p]),
    "pdog_assign_exclusive_host": (_i, [_i, _i, _i, _i, _d, _p, _p, _p, _p, _p, _p]),
    "pdog_detect_chains_exclusive": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _i, _i, _i, _i, _i, _d, _p, _p, _p]),
    "pdog_get_exclusive_counts": (_i, [_p, _pu64]),
}
EXCLUSIVE_SYMBOLS = tuple(EXCLUSIVE_PROTOTYPES)
EXCLUSIVE_MAX_TARGETS = 32   # PDOG_EXCLUSIVE_MAX_TARGETS

# the same for include/pawsome_motion.h, which includes pawsome_exclusive.h: exclusive chains with a motion model
# (tests/test_motion_cpu.py holds this table against that header)
MOTION_PROTOTYPES = {
    "pdog_assign_motion": (_i, [_p, _i, _i, _i, _i, _d, _d, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdog_assign_motion_host": (_i, [_i, _i, _i, _i, _d, _d, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdog_detect_chains_motion": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _i, _i, _i, _i, _i, _d, _d, _i, _p, _p, _p, _p]),
    "pdog_get_motion_counts": (_i, [_p, _pu64]),
}
MOTION_SYMBOLS = tuple(MOTION_PROTOTYPES)
MOTION_MAX_TARGETS = 32      # PDOG_MOTION_MAX_TARGETS

# the same for include/pawsome_predict.h, which includes pawsome_motion.h: one-launch chains with a motion model
# (tests/test_predict_cpu.py holds this table against that header)
PREDICT_PROTOTYPES = {
    "pdog_detect_chains_predicted": (_i, [_p, _p, _i64, _i64, _i, _p, _i, _i, _i, _d, _i, _p, _p, _p, _p]),
    "pdog_get_predict_counts": (_i, [_p, _pu64]),
}
PREDICT_SYMBOLS = tuple(PREDICT_PROTOTYPES)

# the same for include/pawsome_background.h, the fourth header pawsome_dog.h includes: a static background model and frames
# with it subtracted (tests/test_background_cpu.py holds this table against that header)
BACKGROUND_PROTOTYPES = {
    "pdog_bg_create": (_i, [_i, _i, _i, _pp]),
    "pdog_bg_destroy": (_i, [_p]),
    "pdog_bg_samples": (_i, [_p, _i, _i, _p, _i, _pi]),
    "pdog_bg_estimate": (_i, [_p, _p, _p, _i64, _i64, _i, _p, _i]),
    "pdog_bg_set": (_i, [_p, _p, _p, _i64]),
    "pdog_bg_get": (_i, [_p, _p, _p, _i64]),
    "pdog_bg_subtract_indexed": (_i, [_p, _p, _p, _i64, _i64, _i, _p, _i, _p, _i64, _i64]),
}
BACKGROUND_SYMBOLS = tuple(BACKGROUND_PROTOTYPES)
BG_MAX_SAMPLES = 64          # PDOG_BG_MAX_SAMPLES

# the same for include/pawsome_shape.h, the fifth header pawsome_dog.h includes: how a target lies at a tracked position
# (tests/test_shape_cpu.py holds this table against that header)
SHAPE_PROTOTYPES = {
    "pdog_shape": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _i, _i, _p, _p]),
    "pdog_shape_derive": (_i, [_p, _p, _p]),
    "pdog_shape_headings": (_i, [_p, _p, _i, _d, _p]),
}
SHAPE_SYMBOLS = tuple(SHAPE_PROTOTYPES)
SHAPE_MAX_RADIUS = 127       # PDOG_SHAPE_MAX_RADIUS

# the same for include/pawsome_blob.h, a header of its own that includes pawsome_dog.h: the shape of the connected blob under a
# tracked position (tests/test_blob_cpu.py holds this table against that header)
BLOB_PROTOTYPES = {
    "pdog_blob": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _i, _i, _i, _p, _p]),
}
BLOB_SYMBOLS = tuple(BLOB_PROTOTYPES)

# the same for include/pawsome_split.h, a header of its own that includes pawsome_blob.h: every target's blob inside its
# nearest-centre cell (tests/test_split_cpu.py holds this table against that header)
SPLIT_PROTOTYPES = {
    "pdog_blob_split": (_i, [_p, _p, _i64, _i64, _i, _p, _p, _i, _i, _i64, _i64, _i, _i, _i, _p, _p]),
}
SPLIT_SYMBOLS = tuple(SPLIT_PROTOTYPES)
SPLIT_MAX_TARGETS = 32       # PDOG_SPLIT_MAX_TARGETS

# the same for include/pawsome_frame_blobs.h, a header of its own that includes pawsome_dog.h: every connected blob of a whole
# frame (tests/test_frame_blobs_cpu.py holds this table against that header)
FRAME_BLOBS_PROTOTYPES = {
    "pdog_fb_create": (_i, [_i, _i, _i, _i, _pp]),
    "pdog_fb_destroy": (_i, [_p]),
    "pdog_frame_blobs": (_i, [_p, _p, _p, _i64, _i64, _i, _p, _i, _i, _i, _i, _i, _i64, _i64, _i, _p, _p]),
    "pdog_frame_blobs_derive": (_i, [_p, _p]),
}
FRAME_BLOBS_SYMBOLS = tuple(FRAME_BLOBS_PROTOTYPES)
FB_WORDS = 12                # PDOG_FB_WORDS
FB_MAX_IN_FLIGHT = 1024      # PDOG_FB_MAX_IN_FLIGHT

# the same for include/pawsome_refine.h, the sixth header pawsome_dog.h includes: the ranges the pruned strips run, a test hook
# (tests/test_prune_refine_cpu.py holds this table against that header)
REFINE_PROTOTYPES = {
    "pdog_get_prune_jobs": (_i, [_p, _i, _p, _pi]),
}
REFINE_SYMBOLS = tuple(REFINE_PROTOTYPES)
DEFAULT_STOP = 86399.999     # PDOG_DEFAULT_STOP: DEFAULT_MAX_DURATION_SECONDS, src/PawsomeTracker.jl:19


class PdogError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pawsome_dog status {code}: {msg}")
        self.code = code


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 / librccl (same SONAMEs as /opt/rocm's) and opens
    them by path.  If this library were loaded first it would bind to /opt/rocm's copies, `import torch` would then
    bring in a second HIP runtime and a second RCCL, and only the runtime initialised first gets the GPU (seen as
    "no HIP device" from the other).  So when torch is installed it is imported FIRST: its copies are then the ones
    in the process and this library's NEEDED entries resolve to them by SONAME.  (Loading torch's libraries one by
    one instead — as round 1 did for the HIP runtime — breaks their destructor order once librccl is among them:
    `double free` at interpreter exit.)  Without torch nothing happens and /opt/rocm's libraries are used, as for
    any C or Julia host."""
    import sys
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        if importlib.util.find_spec("torch") is None:
            return
        import torch  # noqa: F401
    except (ImportError, ValueError, OSError):
        return


def lib():
    """Load the shared library once; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _preload_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**PROTOTYPES, **VIDEO_PROTOTYPES, **PRUNE_PROTOTYPES, **OVERLAY_PROTOTYPES, **PEAKS_PROTOTYPES,
                                      **EXCLUSIVE_PROTOTYPES, **MOTION_PROTOTYPES, **PREDICT_PROTOTYPES, **BACKGROUND_PROTOTYPES,
                                      **SHAPE_PROTOTYPES, **BLOB_PROTOTYPES, **SPLIT_PROTOTYPES, **FRAME_BLOBS_PROTOTYPES,
                                      **REFINE_PROTOTYPES}.items():
        fn = getattr(L, name, None)     # a symbol the loaded build lacks (an older A/B build through PAWSOME_DOG_LIB) is skipped
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(code):
    if code != PDOG_OK:
        raise PdogError(code, lib().pdog_last_error().decode("utf-8", "replace"))


def new_handle(create, *args):
    """create(*args, &out) checked: the out-pointer the ABI's constructors and getters end with."""
    h = C.c_void_p()
    check(create(*args, C.byref(h)))
    return h


class Handle:
    """One opaque handle of the ABI (`_h`) and the name of the entry point that frees it (None: borrowed, its owner
    frees it).  After close() `_h` is None, which every entry point refuses with PDOG_E_ARG before it launches anything."""
    _h = None

    def __init__(self, h, destroy):
        self._h, self._destroy = h, destroy

    def close(self):
        h, self._h = self._h, None
        if h and self._destroy:
            getattr(lib(), self._destroy)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackerHandle(Handle):
    """A pdog_tracker and the controls that only forward it."""

    def info(self):
        o = PdogInfo()
        check(lib().pdog_get_info(self._h, C.byref(o)))
        return o

    def set_variant(self, variant):
        check(lib().pdog_set_variant(self._h, int(variant)))

    def set_exact(self, on):
        """Exact mode (default on): near-ties of the FP32 ranking are re-decided in the reference's Float64 arithmetic."""
        check(lib().pdog_set_exact(self._h, int(on)))   # 0 off, 1 on, 2 re-evaluate everything (self-check)

    def set_tuning(self, key, value=1):
        """Pin one of the library's alternative code paths (pdog_set_tuning): tests and A/B only."""
        check(lib().pdog_set_tuning(self._h, key.encode(), int(value)))

    def exact_stats(self):
        """(on, threshold 2δ, windows re-evaluated so far) — pdog_get_exact."""
        on, thr, n = C.c_int(), C.c_double(), C.c_uint64()
        check(lib().pdog_get_exact(self._h, C.byref(on), C.byref(thr), C.byref(n)))
        return bool(on.value), thr.value, int(n.value)

    def exact_detail(self):
        """(windows refined, column blocks rescanned, candidates, sequential chains) — pdog_get_exact_detail."""
        out = (C.c_uint64 * 4)()
        check(lib().pdog_get_exact_detail(self._h, out))
        return tuple(int(v) for v in out)

    def prune_counts(self):
        """(kept, total) (strip, sub-chunk) pairs of the batches that ran the bounding pre-pass — pdog_get_prune_counts."""
        out = (C.c_uint64 * 2)()
        check(lib().pdog_get_prune_counts(self._h, out))
        return int(out[0]), int(out[1])

    def peaks_counts(self):
        """(windows detect_peaks served, those among them whose candidate list overflowed) — pdog_get_peaks_counts."""
        out = (C.c_uint64 * 2)()
        check(lib().pdog_get_peaks_counts(self._h, out))
        return int(out[0]), int(out[1])

    def exclusive_counts(self):
        """(joint steps enqueued, times a workspace of the exclusive calls grew) — pdog_get_exclusive_counts."""
        out = (C.c_uint64 * 2)()
        check(lib().pdog_get_exclusive_counts(self._h, out))
        return int(out[0]), int(out[1])

    def motion_counts(self):
        """(motion steps enqueued, times a workspace of the motion calls grew) — pdog_get_motion_counts."""
        out = (C.c_uint64 * 2)()
        check(lib().pdog_get_motion_counts(self._h, out))
        return int(out[0]), int(out[1])

    def predict_counts(self):
        """(launches of the fused kernel's predicted instances, of the persistent chain kernel's, walks handed to the motion
        walk, times the staged table grew) — pdog_get_predict_counts."""
        out = (C.c_uint64 * 4)()
        check(lib().pdog_get_predict_counts(self._h, out))
        return tuple(int(v) for v in out)

    def batch_maxima(self, n):
        """Test hook (not stable ABI): FP32 maxima of the n windows of the last strip-kernel batch (numpy float32 [n]) — pdog_get_batch_maxima."""
        import numpy as np
        out = np.empty(int(n), np.float32)
        check(lib().pdog_get_batch_maxima(self._h, int(n), C.c_void_p(out.ctypes.data)))
        return out

    def prune_jobs(self):
        """Test hook (not stable ABI): the strips the last batch that ran the bounding pre-pass left to compute, numpy int32 [m][4] of
        (window, strip, first 8-row block, one past the last block) in the order they were filed — pdog_get_prune_jobs."""
        import numpy as np
        count = C.c_int()
        check(lib().pdog_get_prune_jobs(self._h, 0, None, C.byref(count)))
        out = np.empty((count.value, 4), np.int32)
        if count.value:
            check(lib().pdog_get_prune_jobs(self._h, count.value, C.c_void_p(out.ctypes.data), C.byref(count)))
        return out[:count.value]

    def kernel_for_batch(self, n):
        """Variant id of the kernel family a batch of n windows runs on (300 fused, 400 tiled, 200 two-pass, else info().variant)."""
        o = C.c_int()
        check(lib().pdog_kernel_for_batch(self._h, int(n), C.byref(o)))
        return o.value

    def reserve(self, n):
        check(lib().pdog_reserve(self._h, int(n)))

    def set_fill(self, fill):
        """The PaddedView fill (src/PawsomeTracker.jl:48) of the launches queued from now on (pdog_set_fill)."""
        check(lib().pdog_set_fill(self._h, int(fill)))

    def sync(self):
        check(lib().pdog_sync(self._h))
