"""Checked arguments of the entry points that take torch tensors.  What these let through reaches a kernel as a raw
pointer with the sizes and strides it indexes by, so a violation is raised (`assert` does not survive `python -O`):
TypeError for a wrong device, dtype or rank, ValueError for a wrong shape, stride or contiguity.  The device is
looked at last, so that everything else about an argument can be judged — and tested — on host tensors."""
import numpy as np

_LAYOUT = {2: "[h, w]", 3: "[n, h, w]", 4: "[n_clips, n_frames, h, w]"}


def _on_device(t, name, device):
    if not t.is_cuda or (device is not None and t.device.index != device):
        raise TypeError(f"{name} must live on the GPU" + ("" if device is None else f" (device {device})") + f", not on {t.device}")
    return t


def device_frames(t, name, dims, hw=None, device=None):
    """Frames as the kernels read them: a uint8 cuda tensor of `dims` dimensions (see _LAYOUT) whose last stride is 1 (the
    row stride may exceed w), clips stacked contiguously, and of the tracker's frame size `hw` where one is given."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != dims:
        raise TypeError(f"{name} must be a uint8 cuda tensor {_LAYOUT[dims]}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: the last stride must be 1, not {t.stride(-1)}")
    if dims == 4 and t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError(f"{name}: clips must be stacked contiguously")
    if hw is not None and (t.shape[-2], t.shape[-1]) != hw:
        raise ValueError(f"{name}: frames of {t.shape[-2]} x {t.shape[-1]}, but the tracker was made for {hw[0]} x {hw[1]}")
    return _on_device(t, name, device)


def device_array(t, name, dtype, shape, device=None):
    """A contiguous cuda tensor of `dtype` and `shape` (None: any size along that axis)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != len(shape):
        raise TypeError(f"{name} must be a {dtype} cuda tensor of {len(shape)} dimension(s)")
    for k, n in enumerate(shape):
        if n is not None and t.shape[k] != n:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple('n' if v is None else v for v in shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return _on_device(t, name, device)


def frame_index_ptr(frame_index, n):
    """None (entry b looks at frame b), or the address of an int32 cuda tensor [n] (n None: any length)."""
    if frame_index is None:
        return None
    import torch
    return device_array(frame_index, "frame_index", torch.int32, (n,)).data_ptr()


def host_i32(v, name, n):
    """n values — None, a sequence, a numpy array or a tensor — as a contiguous host int32 array [n] (None stays None)."""
    if v is None:
        return None
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(v), dtype=np.int32)
    if a.shape != (n,):
        raise ValueError(f"{name}: {n} values expected, one per entry, not shape {a.shape}")
    return a


def peaks_args(k, min_distance, name="k"):
    """The picks per window (1 ... 32, PDOG_PEAKS_MAX_K) and the least distance between two picks (None: the library's
    default, ceil(target_width), passed on as 0; otherwise a positive integer) as pdog_detect_peaks takes them."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {type(k).__name__}")
    if not 1 <= k <= 32:
        raise ValueError(f"{name}: {k} lies outside 1 ... 32")
    if min_distance is None:
        return int(k), 0
    if isinstance(min_distance, bool) or not isinstance(min_distance, (int, np.integer)):
        raise TypeError(f"min_distance must be None or an integer, not {type(min_distance).__name__}")
    if not 1 <= min_distance < 2**31:
        raise ValueError(f"min_distance: {min_distance} is not a positive number of pixels")
    return int(k), int(min_distance)


def exclusive_args(n_targets, k, min_distance, min_ratio):
    """What the exclusive step takes beside its arrays: targets per group 1 ... 32 (PDOG_EXCLUSIVE_MAX_TARGETS), k and
    min_distance as peaks_args judges them — k None: the library's default, min(32, 2 * n_targets), passed on as 0 —, and the
    ratio, a real number in [0, 1].  Returns (k, min_distance, min_ratio) as the library takes them."""
    if not 1 <= n_targets <= 32:
        raise ValueError(f"n_targets: {n_targets} lies outside 1 ... 32")
    k, md = (0, peaks_args(1, min_distance)[1]) if k is None else peaks_args(k, min_distance)
    if isinstance(min_ratio, bool) or not isinstance(min_ratio, (int, float, np.integer, np.floating)):
        raise TypeError(f"min_ratio must be a real number, not {type(min_ratio).__name__}")
    if not 0.0 <= float(min_ratio) <= 1.0:          # (a NaN fails both comparisons)
        raise ValueError(f"min_ratio: {min_ratio} lies outside [0, 1]")
    return k, md, float(min_ratio)


def motion_args(n_targets, k, min_distance, min_ratio, min_response, coast):
    """What the motion step takes beside its arrays: exclusive_args' four, the least response an entry must EXCEED — a finite
    real number >= 0 — and the number of held steps a target keeps its velocity for, an integer >= 0.  Returns (k,
    min_distance, min_ratio, min_response, coast) as the library takes them."""
    k, md, rho = exclusive_args(n_targets, k, min_distance, min_ratio)
    if isinstance(min_response, bool) or not isinstance(min_response, (int, float, np.integer, np.floating)):
        raise TypeError(f"min_response must be a real number, not {type(min_response).__name__}")
    if not 0.0 <= float(min_response) <= 3.4028234663852886e38:    # (it is compared as a float32; a NaN fails both comparisons)
        raise ValueError(f"min_response: {min_response} is not a finite float32 >= 0")
    if isinstance(coast, bool) or not isinstance(coast, (int, np.integer)):
        raise TypeError(f"coast must be an integer, not {type(coast).__name__}")
    if not 0 <= coast < 2**31:
        raise ValueError(f"coast: {coast} is not a number of steps >= 0")
    return k, md, rho, float(min_response), int(coast)


def predict_args(min_response, coast):
    """What the predicted chain takes beside its arrays: min_response and coast as motion_args judges them.  Returns
    (min_response, coast) as the library takes them."""
    return motion_args(1, 1, None, 1.0, min_response, coast)[3:]


def host_table(v, name):
    """A frame table — a sequence of rows, a numpy array or a tensor of integers [n_clips, n_steps] — as a contiguous host int32
    array.  Its entries are the library's to judge (it validates them before it launches anything)."""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name} must hold integers, not {a.dtype}")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name}: shape {a.shape}, expected (n_clips, n_steps)")
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError(f"{name}: entries beyond int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def host_steps(v, name):
    """One row of a frame table — a sequence, a numpy array or a tensor of integers [n_steps] — as a contiguous host int32
    array.  Its entries are the library's to judge, as for host_table."""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.ndim != 1:
        raise ValueError(f"{name}: shape {a.shape}, expected (n_steps,)")
    if a.size == 0:
        return np.zeros(0, np.int32)
    return host_table(a[None, :], name)[0]


def background_k(k, name="k"):
    """A number of background samples: an integer 1 ... 64 (PDOG_BG_MAX_SAMPLES)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {type(k).__name__}")
    if not 1 <= k <= 64:
        raise ValueError(f"{name}: {k} lies outside 1 ... 64")
    return int(k)


def shape_args(radius, min_contrast, prefix=""):
    """What pdog_shape takes beside its arrays: the radius — None: the library's default, ceil(target_width) capped at 127,
    passed on as 0; otherwise an integer 2 ... 127 (PDOG_SHAPE_MAX_RADIUS) — and the least contrast of a target, an integer
    1 ... 255.  Returns (radius, min_contrast) as the library takes them; `prefix` goes in front of the names in a message."""
    rn, cn = prefix + "radius", prefix + "min_contrast"
    if radius is None:
        radius = 0
    elif isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise TypeError(f"{rn} must be None or an integer, not {type(radius).__name__}")
    elif not 2 <= radius <= 127:
        raise ValueError(f"{rn}: {radius} lies outside 2 ... 127")
    if isinstance(min_contrast, bool) or not isinstance(min_contrast, (int, np.integer)):
        raise TypeError(f"{cn} must be an integer, not {type(min_contrast).__name__}")
    if not 1 <= min_contrast <= 255:
        raise ValueError(f"{cn}: {min_contrast} lies outside 1 ... 255")
    return int(radius), int(min_contrast)


def blob_args(radius, min_contrast, connectivity, prefix=""):
    """What pdog_blob takes beside its arrays: shape_args' two and the connectivity, the integer 4 (edge neighbours) or 8
    (edge and corner neighbours).  Returns (radius, min_contrast, connectivity) as the library takes them."""
    radius, min_contrast = shape_args(radius, min_contrast, prefix)
    name = prefix + "connectivity"
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)):
        raise TypeError(f"{name} must be the integer 4 or 8, not {type(connectivity).__name__}")
    if connectivity not in (4, 8):
        raise ValueError(f"{name}: {connectivity} is neither 4 nor 8")
    return radius, min_contrast, int(connectivity)


def _integer(v, name, lo, hi, what=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {type(v).__name__}")
    if not lo <= v <= hi:
        raise ValueError(f"{name}: {v} " + (what or f"lies outside {lo} ... {hi}"))
    return int(v)


def frame_blobs_args(n_pix, level, darker_target, min_contrast, connectivity, min_area, max_area, cap):
    """What pdog_frame_blobs takes beside its arrays, for frames of n_pix pixels: the level 0 ... 255, the sign (True or False),
    the least contrast 1 ... 255, the connectivity 4 or 8, the area limits 1 <= min_area <= max_area (None: n_pix) and the number
    of rows per step, cap >= 1.  Returns (level, darker, min_contrast, connectivity, min_area, max_area, cap) as the library
    takes them."""
    level = _integer(level, "level", 0, 255)
    if not isinstance(darker_target, (bool, np.bool_)):
        raise TypeError(f"darker_target must be True or False, not {type(darker_target).__name__}")
    min_contrast = _integer(min_contrast, "min_contrast", 1, 255)
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)):
        raise TypeError(f"connectivity must be the integer 4 or 8, not {type(connectivity).__name__}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity: {connectivity} is neither 4 nor 8")
    min_area = _integer(min_area, "min_area", 1, 2**62, "is not an area >= 1")
    max_area = int(n_pix) if max_area is None else _integer(max_area, "max_area", min_area, 2**62, f"lies below min_area = {min_area}")
    cap = _integer(cap, "cap", 1, 2**31 - 1, "is not a number of rows >= 1")
    return level, int(bool(darker_target)), min_contrast, int(connectivity), min_area, max_area, cap


def host_samples(v, name):
    """The sample list of a background estimate: host_steps' row, of 1 ... 64 entries.  The entries are the library's to judge."""
    a = host_steps(v, name)
    if not 1 <= len(a) <= 64:
        raise ValueError(f"{name}: {len(a)} samples, 1 ... 64 expected")
    return a


def device_positions(t, name, n_steps, device=None):
    """Positions of several targets as the overlay reads them: an int32 cuda tensor [n_targets, n_steps, 2] whose pairs and steps
    lie densely (strides 1 and 2) and whose targets lie an even number of words >= 2 * n_steps apart — a column slice
    out[:, k0:k1] of a chains result as it lies.  Returns the distance between two targets in positions."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 3:
        raise TypeError(f"{name} must be an int32 cuda tensor [n_targets, n_steps, 2]")
    if t.shape[0] < 1 or t.shape[1] != n_steps or t.shape[2] != 2:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected (n_targets, {n_steps}, 2)")
    if t.stride(2) != 1 or (n_steps > 1 and t.stride(1) != 2):
        raise ValueError(f"{name}: pairs and steps must lie densely (strides 2 and 1), not {t.stride(1)} and {t.stride(2)}")
    stride = t.stride(0) if t.shape[0] > 1 else max(2 * n_steps, 2)      # (one target: the stride is never used)
    if stride < 2 * n_steps or stride % 2:
        raise ValueError(f"{name}: targets must lie an even number of words >= {2 * n_steps} apart, not {stride}")
    _on_device(t, name, device)
    return stride // 2
