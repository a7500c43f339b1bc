"""The frame-blob rule (include/pawsome_frame_blobs.h) as far as no GPU is needed: the header against
_lib.FRAME_BLOBS_PROTOTYPES and the library's exports, the header alone under a C and a C++ compiler, the binding's argument
checks on host tensors, the kernels' host-only pieces and their steps replayed in a stand-alone program
(tests/frame_blobs_main.cpp, built plain and with AddressSanitizer and UBSan), the admitted frame sizes (the header's "Sizes")
of that program, of the binding and of pdog_fb_create against the rule in Python integers at the edge of thirteen widths, the
restatement's int64 sums and the derived values at the two largest admitted sizes, pdog_frame_blobs_derive through the library
against NumPy on drawn ellipses, the restatement (tests/frame_blobs_restatement.py, which the GPU must equal bit for bit:
tests/test_gpu_frame_blobs.py) against a plain pixel flood fill on every scene of tests/frame_blobs_scenes.py, what the scenes
claim to contain, and — on the oracle alone — the bootstrap scene: three discs outside the centre window, of which today's
n_targets rule finds none and the frame rule all three."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _args, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_blobs_restatement as FR  # noqa: E402
import frame_blobs_scenes as FS  # noqa: E402
import peaks_restatement as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "pawsome_frame_blobs.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
NAMES = ["pdog_fb_create", "pdog_fb_destroy", "pdog_frame_blobs", "pdog_frame_blobs_derive"]


# ---- the kernels' host-only pieces under the host compiler ----
BUILDS = pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
_EXES = {}


def _program(tmp_path_factory, flags):
    """tests/frame_blobs_main.cpp under the host compiler, built once per set of flags for the tests of this file."""
    if flags not in _EXES:
        exe = tmp_path_factory.mktemp("frame_blobs") / "frame_blobs"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                               os.path.join(ROOT, "tests", "frame_blobs_main.cpp"), "-o", str(exe)])
        _EXES[flags] = str(exe)
    return _EXES[flags]


@BUILDS
def test_kernel_steps_replayed_on_the_host_match_the_flood_fill(tmp_path_factory, flags):
    p = subprocess.run([_program(tmp_path_factory, flags)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert re.search(r"\b[1-9][0-9]* checks, 0 mismatches", p.stdout) and "1120 frames replayed" in p.stdout


# ---- the admitted frame sizes ----
T = lambda k: k * (k - 1) // 2  # noqa: E731
S2 = lambda k: (k - 1) * k * (2 * k - 1) // 6  # noqa: E731
MOST = 2**63 - 1
EDGE_WIDTHS = (1, 2, 3, 63, 64, 65, 520, 1920, 3840, 16384, 32768, 2**21 - 1, 2**21)


def _rule(h, w):
    """The header's "Sizes" in Python integers: None for an admitted size, otherwise what does not fit."""
    checks = ((h >= 1 and w >= 1, "a side is not positive"), (h * w <= 2**30, "more than 2^30 pixels"),
              (w <= _lib.PDOG_MAX_ROW_STRIDE, "frame_w exceeds PDOG_MAX_ROW_STRIDE"), (w * S2(h) <= MOST, "Syy of a full frame leaves 63 bits"),
              (h * S2(w) <= MOST, "Sxx of a full frame leaves 63 bits"), (T(h) * T(w) <= MOST, "Syx of a full frame leaves 63 bits"))
    return next((text for ok, text in checks if not ok), None)


def _largest_h(w):
    lo, hi = 0, 2**31                      # admitted sizes are downward closed in h: every word grows with h
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _rule(mid, w) is None else (lo, mid)
    return lo


def _full_words(h, w):
    return [h * w, w * T(h), h * T(w), w * S2(h), T(h) * T(w), h * S2(w), 0, h - 1, 0, w - 1, 0]


def test_the_header_s_table_of_largest_heights_is_the_rule_s():
    table = {1: 3024617, 2: 2400640, 64: 756154, 1920: 243353, 3840: 193149, 16384: 65536, 32768: 32768, 2**21: 3}
    assert {w: _largest_h(w) for w in table} == table
    assert _rule(65537, 16384) == _rule(32769, 32768) == "more than 2^30 pixels"      # where the pixel limit binds first
    text = " ".join(open(HDR).read().replace(" *", " ").split())
    assert "No word of a frame below 2^30 pixels" not in text and "ADMITTED" in text
    assert "w 1 2 64 1920 3840 16 384 32 768 2^21 h " + " ".join(f"{x:,}".replace(",", " ") for x in table.values()) in text  # its small table
    assert "3 024 617" in inspect.getdoc(pt.FrameBlobs) and "2^63 - 1" in inspect.getdoc(pt.FrameBlobs)


@BUILDS
def test_size_rule_of_the_library_equals_python_integers(tmp_path_factory, flags):
    from pawsometracker_jl_amd.frame_blobs import frame_size_refusal
    cases = []
    for w in EDGE_WIDTHS:
        h = _largest_h(w)
        assert h >= 1 and _rule(h, w) is None and _rule(h + 1, w) is not None
        cases += [(h, w), (h + 1, w)]
    cases.append((1, 2**21 + 1))
    cases += [(w, h) for h, w in cases if h * w <= 2**30]                   # the transposes that the pixel limit allows
    cases += [(0, 5), (5, 0), (-1, -1), (2**31 - 1, 2**31 - 1), (2**40, 2**40), (2**62, 4), (-2**63, 3)]
    assert len(set(cases)) > 45 and {_rule(h, w) for h, w in cases} >= {None, "more than 2^30 pixels", "frame_w exceeds PDOG_MAX_ROW_STRIDE",
                                                                         "Syy of a full frame leaves 63 bits", "Sxx of a full frame leaves 63 bits"}
    p = subprocess.run([_program(tmp_path_factory, flags), "sizes"], input="".join(f"{h} {w}\n" for h, w in cases), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    want = [f"{h} {w} " + ("admitted" if _rule(h, w) is None else "refused: " + _rule(h, w)) for h, w in cases]
    assert p.stdout.splitlines() == want
    for h, w in cases:                                                      # and the binding's mirror
        assert frame_size_refusal(h, w) == _rule(h, w), (h, w)


def test_refused_sizes_are_refused_without_a_device():
    L = pt.lib()
    for w, text in ((1, "Syy"), (1920, "Syy"), (2**21, "Sxx")):
        h = _largest_h(w) + 1
        out = C.c_void_p(1)
        assert L.pdog_fb_create(0, h, w, 1, C.byref(out)) == _lib.PDOG_E_ARG and not out.value
        msg = L.pdog_last_error().decode()
        assert msg.startswith(f"pdog_fb_create: bad frame size {h} x {w}: ") and text in msg, msg
        with pytest.raises(ValueError, match=f"{h} x {w}.*{text}"):
            pt.FrameBlobs(h, w)
    assert L.pdog_fb_create(0, 1, 2**21 + 1, 1, C.byref(out)) == _lib.PDOG_E_ARG and b"PDOG_MAX_ROW_STRIDE" in L.pdog_last_error()
    with pytest.raises(ValueError, match="PDOG_MAX_ROW_STRIDE"):
        pt.FrameBlobs(1, 2**21 + 1)


@pytest.mark.parametrize("h,w", [(3024617, 1), (3, 2**21)])
def test_restatement_and_derive_hold_at_the_largest_admitted_sizes(h, w):
    assert _rule(h, w) is None and (_rule(h + 1, w) is not None) and max(_full_words(h, w)) > 0.999999 * 2**63
    # the restatement's int64 sums do not wrap on the full frame
    frame = FS.draw(FS.pattern("full", h, w))
    words, n_mask = FR.all_blobs(frame, connectivity=4)
    assert n_mask == h * w and len(words) == 1 and words[0, :11].tolist() == _full_words(h, w)
    assert int(words[0, FR.SS]) == int((128 - frame.astype(np.int64)).sum())
    # the derived values of the closed forms.  The axes come from mxx + myy -+ hypot(0, mxx - myy), with the larger moment
    # L^2 / 12, L = max(h, w): one ulp of it (2^-13 at L = 3 024 617) is what the SHORT axis, 4 sqrt(1/12 ...), is known to,
    # about 1e-3 — inside the 4K case's bound of 1e-9 L.  Nothing is cancelled in the other values.
    got = pt.frame_blobs_derive(np.array(_full_words(h, w) + [0], np.int64))
    long_, short = max(h, w), min(h, w)
    want = np.array([(h + 1) / 2, (w + 1) / 2, np.pi / 2 if h > w else 0.0, 4 * np.sqrt(long_ * long_ / 12), 4 * np.sqrt(short * short / 12),
                     2 * np.sqrt(h * w / np.pi)])
    assert np.abs(got - want).max() <= 1e-9 * long_, (got, want)
    assert np.abs(got[[0, 1, 3, 5]] - want[[0, 1, 3, 5]]).max() <= 1e-12 * long_, (got, want)
    assert np.array_equal(got, FR.derive(_full_words(h, w) + [0])) or np.abs(got - FR.derive(_full_words(h, w) + [0])).max() <= 1e-12 * long_


# ---- the header, the table, the exports ----
def _prototypes(path):
    hdr = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    out = []
    for stmt in hdr.split(";"):
        m = re.search(r"\bint\s+(pdog_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            out.append((m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]))
    return out


def test_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.FRAME_BLOBS_PROTOTYPES) == list(_lib.FRAME_BLOBS_SYMBOLS) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.FRAME_BLOBS_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    args = dict(protos)["pdog_frame_blobs"]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "fb", "hip_stream", "d_frames", "frame_stride", "row_stride", "n_frames", "h_table", "n_steps", "level", "darker",
        "min_contrast", "connectivity", "min_area", "max_area", "cap", "d_out_words", "d_out_count"]
    # the stack's arguments are pdog_bg_subtract_indexed's
    bg = dict(_prototypes(os.path.join(INC, "pawsome_background.h")))["pdog_bg_subtract_indexed"]
    assert args[1:8] == bg[1:8]
    text = open(HDR).read()
    assert '#include "pawsome_dog.h"' in text and "LOWERS A LABEL OR ENDS" in text and "64-bit because" in text
    assert "scipy.ndimage.label" in text and "this library's choice" in text and _lib.FB_WORDS == 12
    assert re.search(r"#define PDOG_FB_WORDS 12\b", text) and re.search(rf"#define PDOG_FB_MAX_IN_FLIGHT {_lib.FB_MAX_IN_FLIGHT}\b", text)
    # a header of its own: pawsome_dog.h stays as it is and does not include it
    assert "pawsome_frame_blobs.h" not in open(os.path.join(INC, "pawsome_dog.h")).read()
    assert pt.lib().pdog_abi_version() == 1


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_frame_blobs.h"\n'
                   "int use(pdog_fb *fb, const uint8_t *f, const int32_t *t, int64_t *w, int32_t *c, double *o) {\n"
                   "    return pdog_frame_blobs(fb, 0, f, 0, 1, 1, t, 1, 128, 1, 8, 8, 1, 1, PDOG_FB_MAX_IN_FLIGHT, w, c)\n"
                   "           + pdog_frame_blobs_derive(w, o) + PDOG_FB_WORDS;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", HDR])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", HDR])


# ---- the binding ----
def test_new_keyword_class_and_methods():
    par = inspect.signature(pt.track_video).parameters
    names = list(par)
    assert par["find"].default == "window" and names[names.index("min_distance") + 1] == "find"
    par = inspect.signature(pt.FrameBlobs.__init__).parameters
    assert list(par)[1:] == ["frame_h", "frame_w", "device", "steps_in_flight"] and par["device"].default == 0
    par = inspect.signature(pt.FrameBlobs.find).parameters
    assert list(par)[1:] == ["frames", "table", "level", "darker_target", "min_contrast", "connectivity", "min_area", "max_area", "cap"]
    assert [par[k].default for k in list(par)[2:]] == [None, 128, True, 8, 8, 1, None, 64]
    assert issubclass(pt.FrameBlobs, _lib.Handle) and hasattr(pt.FrameBlobs, "__enter__") and callable(pt.frame_blobs_derive)


def test_python_argument_checks():
    import torch
    ok = dict(level=128, darker_target=True, min_contrast=8, connectivity=8, min_area=1, max_area=None, cap=64)
    assert _args.frame_blobs_args(100, **ok) == (128, 1, 8, 8, 1, 100, 64)
    assert _args.frame_blobs_args(100, np.int64(0), np.bool_(False), np.int32(255), np.int32(4), np.int64(7), 7, np.int32(1)) == (0, 0, 255, 4, 7, 7, 1)
    bad = [(TypeError, "level", 128.0), (TypeError, "level", True), (ValueError, "level", -1), (ValueError, "level", 256),
           (TypeError, "darker_target", 1), (TypeError, "darker_target", None),
           (TypeError, "min_contrast", "8"), (ValueError, "min_contrast", 0), (ValueError, "min_contrast", 256),
           (TypeError, "connectivity", 8.0), (TypeError, "connectivity", None), (ValueError, "connectivity", 6), (ValueError, "connectivity", 0),
           (TypeError, "min_area", 1.0), (ValueError, "min_area", 0), (ValueError, "min_area", -3),
           (TypeError, "max_area", 5.0), (ValueError, "max_area", 0), (TypeError, "cap", None), (ValueError, "cap", 0)]
    for exc, name, v in bad:
        with pytest.raises(exc, match=name) as e:
            _args.frame_blobs_args(100, **{**ok, name: v})
        assert type(e.value) is exc, (name, v)
    with pytest.raises(ValueError, match="max_area: 4 lies below min_area = 5"):
        _args.frame_blobs_args(100, **{**ok, "min_area": 5, "max_area": 4})
    # the constructor judges its sizes before it asks for a device
    for exc, a in ((TypeError, (10.0, 10)), (TypeError, (10, True)), (ValueError, (0, 10)), (ValueError, (10, -1)), (ValueError, (1 << 16, 1 << 15))):
        with pytest.raises(exc, match="frame"):
            pt.FrameBlobs(*a)
    for exc, s in ((TypeError, 2.0), (ValueError, 0), (ValueError, _lib.FB_MAX_IN_FLIGHT + 1)):
        with pytest.raises(exc, match="steps_in_flight"):
            pt.FrameBlobs(10, 10, steps_in_flight=s)
    # track_video: find is judged before the frames are looked at
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for kw in (dict(find="frame"), dict(find="blob", n_targets=2), dict(find=None, n_targets=2), dict(find=1, n_targets=2)):
        with pytest.raises(ValueError, match="find") as e:
            pt.track_video(frames, 30, **kw)
        assert type(e.value) is ValueError, kw
    with pytest.raises(TypeError, match="cuda tensor"):
        pt.track_video(frames, 30, n_targets=2, find="frame")
    with pytest.raises(TypeError, match="cuda tensor"):
        pt.track_video(frames, 30, n_targets=2, find="window")
    # the library refuses before any GPU call: a null handle, null pointers to derive
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    t, w, c = np.zeros(1, np.int32), np.zeros(12, np.int64), np.zeros(2, np.int32)
    assert pt.lib().pdog_frame_blobs(None, None, P(w), 0, 1, 1, P(t), 1, 128, 1, 8, 8, 1, 1, 1, P(w), P(c)) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_last_error().startswith(b"pdog_frame_blobs: null handle")
    assert pt.lib().pdog_frame_blobs_derive(None, P(np.zeros(6))) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_fb_create(0, 0, 5, 1, C.byref(C.c_void_p())) == _lib.PDOG_E_ARG and b"0 x 5" in pt.lib().pdog_last_error()
    assert pt.lib().pdog_fb_create(0, 5, 5, 0, C.byref(C.c_void_p())) == _lib.PDOG_E_ARG and b"steps_in_flight 0" in pt.lib().pdog_last_error()
    assert pt.lib().pdog_fb_destroy(None) == _lib.PDOG_OK
    for exc, v in ((TypeError, np.zeros((2, 12))), (ValueError, np.zeros((2, 11), np.int64)), (ValueError, np.int64(3))):
        with pytest.raises(exc, match="words"):
            pt.frame_blobs_derive(v)
    assert pt.frame_blobs_derive(np.zeros((0, 12), np.int64)).shape == (0, 6)


# ---- pdog_frame_blobs_derive against NumPy on drawn ellipses ----
def _ellipse(h, w, cy, cx, a, b, theta):
    yy, xx = np.mgrid[0:h, 0:w].astype(float)
    u = (xx - cx) * np.cos(theta) + (yy - cy) * np.sin(theta)
    v = -(xx - cx) * np.sin(theta) + (yy - cy) * np.cos(theta)
    return u * u / (a * a) + v * v / (b * b) <= 1.0


def test_derive_equals_numpy_on_drawn_ellipses():
    rng = np.random.default_rng(20261021)
    n_seen = 0
    for k in range(60):
        h, w = (120, 160) if k % 20 else (2160, 3840)                # small frames, and sums of a 4K frame's size
        big = 1 if k % 20 else 12
        a, b = big * rng.uniform(6, 30), big * rng.uniform(2, 6)
        cy, cx, theta = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w, rng.uniform(-1.5, 1.5)
        m = _ellipse(h, w, cy, cx, a, b, theta)
        words, n_mask = FR.all_blobs(np.where(m, 60, 128).astype(np.uint8))
        assert len(words) == 1 and words[0, FR.N] == n_mask == m.sum()
        got = pt.frame_blobs_derive(words)[0]
        rr, cc = (v.astype(np.float64) for v in np.nonzero(m))
        my, mx = rr.mean(), cc.mean()
        myy, mxx, myx = ((rr - my) ** 2).mean() + 1 / 12, ((cc - mx) ** 2).mean() + 1 / 12, ((rr - my) * (cc - mx)).mean()
        t = np.hypot(2 * myx, mxx - myy)
        want = np.array([1 + my, 1 + mx, 0.5 * np.arctan2(2 * myx, mxx - myy), 4 * np.sqrt((mxx + myy + t) / 2),
                         4 * np.sqrt(max((mxx + myy - t) / 2, 0.0)), 2 * np.sqrt(m.sum() / np.pi)])
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (k, got, want)
        assert np.array_equal(got, FR.derive(words)[0], equal_nan=True) or np.abs(got - FR.derive(words)[0]).max() <= 1e-12
        # the drawn ellipse comes back: centre within half a pixel, direction within a few degrees, axes within a pixel or 3 %
        assert abs(got[0] - 1 - cy) < 0.5 and abs(got[1] - 1 - cx) < 0.5 and abs(np.angle(np.exp(2j * (got[2] - theta)))) < 0.2
        assert abs(got[3] - 2 * a) < max(1.0, 0.06 * a) and abs(got[4] - 2 * b) < max(1.0, 0.06 * b)
        n_seen += 1
    assert n_seen == 60
    # a blob whose Syy needs more than 32 bits, and numerators that need more than 64: the whole 4K frame
    h, w = 2160, 3840
    n, sy, sx = h * w, w * (h - 1) * h // 2, h * (w - 1) * w // 2
    syy, sxx, syx = w * (h - 1) * h * (2 * h - 1) // 6, h * (w - 1) * w * (2 * w - 1) // 6, ((h - 1) * h // 2) * ((w - 1) * w // 2)
    assert syy > 2**32 and n * syy > 2**63
    got = pt.frame_blobs_derive(np.array([n, sy, sx, syy, syx, sxx, 0, h - 1, 0, w - 1, 0, 0], np.int64))
    want = [1 + (h - 1) / 2, 1 + (w - 1) / 2, 0.0, 4 * np.sqrt(w * w / 12), 4 * np.sqrt(h * h / 12), 2 * np.sqrt(n / np.pi)]
    assert np.abs(got - want).max() <= 1e-9 * w
    assert np.isnan(pt.frame_blobs_derive(np.zeros(12, np.int64))).all()


# ---- the restatement against a plain pixel flood fill ----
def _flood_words(frame, level, darker, min_contrast, connectivity):
    s = FR.contrast(frame, level, darker)
    mask = s >= min_contrast
    h, w = mask.shape
    seen = np.zeros_like(mask)
    out = []
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for r0, c0 in zip(*np.nonzero(mask)):                              # raster order: a blob is met at its first pixel
        if seen[r0, c0]:
            continue
        seen[r0, c0] = True
        stack, px = [(int(r0), int(c0))], []
        while stack:
            r, c = stack.pop()
            px.append((r, c))
            for dr, dc in nb:
                rr, cc = r + dr, c + dc
                if 0 <= rr < h and 0 <= cc < w and mask[rr, cc] and not seen[rr, cc]:
                    seen[rr, cc] = True
                    stack.append((rr, cc))
        R, Cc = (np.array(v, np.int64) for v in zip(*px))
        out.append([len(px), R.sum(), Cc.sum(), (R * R).sum(), (R * Cc).sum(), (Cc * Cc).sum(), R.min(), R.max(), Cc.min(), Cc.max(),
                    int(r0) * w + int(c0), int(s[R, Cc].sum())])
    return np.array(out, np.int64).reshape(-1, 12), int(mask.sum())


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_the_flood_fill_on_every_scene(connectivity):
    n_blobs = 0
    for h, w in ((1, 1), (2, 63), (31, 65), (33, 129), (70, 64), (70, 200)):
        for darker in (True, False):
            stack = FS.frames(h, w, darker)
            for k, name in enumerate(FS.NAMES):
                got, n_mask = FR.all_blobs(stack[k], FS.LEVEL[darker], darker, 8, connectivity)
                want, want_mask = _flood_words(stack[k], FS.LEVEL[darker], darker, 8, connectivity)
                assert n_mask == want_mask == FS.pattern(name, h, w).sum(), (name, h, w)
                assert np.array_equal(got, want), (name, h, w, darker)
                assert (np.diff(got[:, FR.FIRST]) > 0).all()
                n_blobs += len(got)
    assert n_blobs > 1000
    # find: the filter, the cut list and the zero rows behind it, the table
    stack = FS.frames(33, 129)
    k = FS.NAMES.index("noise 0.41")
    w_all, n_mask = FR.all_blobs(stack[k], connectivity=connectivity)
    count, words = FR.find(stack, [k, 0, k], connectivity=connectivity, min_area=3, max_area=9, cap=7)
    kept = w_all[(w_all[:, 0] >= 3) & (w_all[:, 0] <= 9)]
    assert len(kept) > 7 and count.tolist() == [[len(kept), n_mask], [0, 0], [len(kept), n_mask]]
    assert np.array_equal(words[0], kept[:7]) and not words[1].any() and np.array_equal(words[2], words[0])
    count, words = FR.find(stack, [k], connectivity=connectivity, min_area=3, max_area=9, cap=len(kept) + 2)
    assert np.array_equal(words[0, :len(kept)], kept) and not words[0, len(kept):].any()


def test_scenes_contain_what_they_claim():
    h, w = 70, 200
    blobs = lambda name, conn, hw=(h, w): FR.all_blobs(FS.draw(FS.pattern(name, *hw)), connectivity=conn)[0]  # noqa: E731
    assert len(blobs("empty", 8)) == 0 and len(blobs("full", 4)) == 1 and blobs("full", 4)[0, 0] == h * w
    assert blobs("corners", 8)[:, FR.FIRST].tolist() == [0, w - 1, (h - 1) * w, h * w - 1]
    for hw in ((70, 200), (33, 129), (31, 63)):
        for conn in (4, 8):                                    # one blob that is as long as half the frame
            sp = blobs("spiral", conn, hw)
            assert len(sp) == 1 and sp[0, 0] > hw[0] * hw[1] // 2 - 2 * (hw[0] + hw[1]), (hw, conn, sp[:, 0])
            assert len(blobs("comb", conn, hw)) == 1 and len(blobs("lattice", conn, hw)) == 1
    assert len(blobs("checkerboard", 8)) == 1 and len(blobs("checkerboard", 4)) == h * w // 2 > 64
    st8, st4 = blobs("staircases", 8), blobs("staircases", 4)
    # at 8 the two crossing diagonals are one blob and the third another; at 4 every pixel is alone but the 2 x 2 of the crossing
    assert len(st8) == 2 and len(st4) == st8[:, 0].sum() - 3 and sorted(st4[:, 0].tolist())[-2:] == [1, 4]
    m = FS.pattern("staircases", h, w)
    assert m[63, 63] and m[64, 64] and m[63, 64] and m[64, 63]              # through the tile corners, both ways
    for conn in (4, 8):                                                     # the bars one pixel apart stay apart
        nb = blobs("neighbours", conn)
        assert len(nb) == 6 and nb[:, FR.CMIN].tolist().count(62) == 1 and (nb[:, 0] > 30).all()
    for name in ("noise 0.41", "noise 0.59"):
        assert len(blobs(name, 4)) > 64 and len(blobs(name, 4)) > len(blobs(name, 8))
    assert len(blobs("noise 0.41", 8)) > 64 > len(blobs("noise 0.59", 8))                       # (above both thresholds: nearly one blob)
    assert blobs("noise 0.59", 4)[:, 0].max() > 1000 > blobs("noise 0.41", 4)[:, 0].max()       # 4: below and above 0.593
    assert blobs("noise 0.41", 8)[:, 0].max() > 1000                                             # 8: above 0.407


# ---- the bootstrap scene, on the oracle alone ----
def test_bootstrap_scene_window_rule_finds_none_frame_rule_finds_all(oracle):
    video, _ = FS.boot_video()
    tw, h, w = FS.BOOT_TW, FS.BOOT_H, FS.BOOT_W
    f0 = video[0]
    fill = oracle.mode_u8(f0)
    assert fill == 128
    # today's rule: the peaks of the sz .÷ 4 window around the centre — on this frame, flat inside the window's reach
    K = oracle.dog_kernel(oracle.sigma(tw), True)
    radii, guess = ((h // 4) // 2, (w // 4) // 2), (h // 2, w // 2)
    pos, R64 = oracle.detect(f0, fill, K, radii, guess, want_resp=True)
    _, peak, count = PR.select(R64, guess, radii, (h, w), pos, 3, PR.default_min_distance(tw))
    on_a_disc = float(oracle.detect(f0, fill, K, (3, 3), tuple(FS.boot_centres(0)[0]), want_resp=True)[1].max())
    # (the oracle's Float64 sums leave ~1e-16 on a flat window where the kernels leave exactly 0: positive means above that)
    assert on_a_disc > 0.01 and (peak[:count] > 1e-9 * on_a_disc).sum() == 0 < 3
    # the frame rule
    guesses, kept = FR.start_guesses(f0, fill, True, tw, 3)
    assert kept == 3 and FR.start_area_limits(tw) == (24, 363)
    assert np.abs(np.array(guesses) - FS.boot_centres(0)).max() <= 1
    assert [int(FR.all_blobs(f0)[0][i, 0]) for i in (0, 1, 2)] == [113, 49, 81]            # in raster order …
    assert guesses == [tuple(c) for c in FS.boot_centres(0)]                                  # … and by size: target 0 is the largest
    # refined like a given start location: the functor at the guess
    ws = pt.fix_window_size(pt.guess_window_size(tw))
    starts = [tuple(oracle.detect(f0, fill, K, (ws[0] // 2, ws[1] // 2), g)) for g in guesses]
    assert np.abs(np.array(starts) - FS.boot_centres(0)).max() <= 1
    # fewer kept blobs than asked for; and the furniture: on the raw frame the slab is too large to be an animal, but the stain
    # (360 pixels) passes for the largest one — under the background both are gone
    assert FR.start_guesses(f0, fill, True, tw, 4)[1] == 3
    cluttered, arena = FS.boot_video(furniture=True)
    raw, kept = FR.start_guesses(cluttered[0], 128, True, tw, 3)
    assert kept == 4 and raw == [(106, 136)] + guesses[:2]
    sub = np.clip(128 + cluttered.astype(int) - arena.astype(int), 0, 255).astype(np.uint8)
    assert np.array_equal(sub, video)
