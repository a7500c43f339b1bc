"""The overlay over a frame table and for several targets (include/pawsome_overlay.h) as far as no GPU is needed: the third
header against _lib.OVERLAY_PROTOTYPES and the library's exports, either header alone as C99 and as C++, the restatement
(tests/overlay_restatement.py) against diag_restatement where the two must agree, and the Python-side argument checks."""
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
import diag_restatement as R  # noqa: E402
import overlay_restatement as OR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY_HDR = os.path.join(ROOT, "include", "pawsome_overlay.h")
NAMES = {"pdog_diag_set_targets", "pdog_diag_get_targets", "pdog_diag_render_indexed"}


def _prototypes(path):
    """[(name, [argument declarations])] of the `int pdog_*(...)` prototypes of a header, comments and directives removed."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    out = []
    for stmt in hdr.split(";"):
        m = re.search(r"\bint\s+(pdog_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            out.append((m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]))
    return out


def test_overlay_symbols_are_declared_bound_and_exported():
    assert {name for name, _ in _prototypes(OVERLAY_HDR)} == set(_lib.OVERLAY_SYMBOLS) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        fn = getattr(pt.lib(), name)
        restype, argtypes = _lib.OVERLAY_PROTOTYPES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    hdr = open(OVERLAY_HDR).read()
    assert "#define PDOG_DIAG_MAX_TARGETS 1024" in hdr and pt.DIAG_MAX_TARGETS == _lib.DIAG_MAX_TARGETS == 1024
    main = open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
    assert main.index('#include "pawsome_overlay.h"') > main.index("int pdog_diag_render")     # at its end
    for name in ("set_targets", "targets", "render_indexed"):
        assert hasattr(pt.Diagnose, name), name
    for fn, kws in ((pt.track_video, ("diagnostic", "diagnostic_chunk")),
                    (pt.track_clips, ("diagnostic", "diagnostic_clips", "diagnostic_chunk"))):
        par = inspect.signature(fn).parameters
        assert all(k in par for k in kws), fn
        assert par["diagnostic"].default is None and par["diagnostic_chunk"].default == 256


def test_overlay_prototype_table_matches_the_header():
    """Argument by argument, as tests/test_video_cpu.py holds its table: an int64_t stride bound as c_int would be truncated
    without a word."""
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    protos = _prototypes(OVERLAY_HDR)
    assert [name for name, _ in protos] == list(_lib.OVERLAY_PROTOTYPES)
    for name, args in protos:
        restype, argtypes = _lib.OVERLAY_PROTOTYPES[name]
        assert restype is C.c_int and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert len(dict(protos)["pdog_diag_render_indexed"]) == 14


def test_abi_version_is_unchanged():
    assert pt.lib().pdog_abi_version() == 1


def test_either_header_compiles_alone(tmp_path):
    """A C host includes pawsome_dog.h and nothing else and has the new calls; pawsome_overlay.h alone compiles too."""
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_dog.h"\n'
                   "int use(pdog_diag *d, const uint8_t *f, const int32_t *tab, const int32_t *ij, uint8_t *out, int *n) {\n"
                   "    return pdog_diag_set_targets(d, PDOG_DIAG_MAX_TARGETS) + pdog_diag_get_targets(d, n)\n"
                   "         + pdog_diag_render_indexed(d, 0, f, 0, 0, 1, 1, 1, tab, 1, ij, 1, 1, out);\n}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", inc, str(src)])
    for hdr in (OVERLAY_HDR, os.path.join(inc, "pawsome_dog.h")):
        subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", hdr])
        subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", hdr])


def test_entry_points_refuse_a_null_handle():
    L = pt.lib()
    n = C.c_int(-77)
    tab = np.zeros(2, np.int32)
    assert L.pdog_diag_set_targets(None, 2) == _lib.PDOG_E_ARG and L.pdog_last_error().startswith(b"pdog_diag_set_targets")
    assert L.pdog_diag_get_targets(None, C.byref(n)) == _lib.PDOG_E_ARG and n.value == -77
    assert L.pdog_diag_render_indexed(None, None, None, 0, 0, 1, 1, 1, C.c_void_p(tab.ctypes.data), 2, None, 2, 1, None) == _lib.PDOG_E_ARG
    assert L.pdog_last_error().startswith(b"pdog_diag_render_indexed")


# ---- the restatement ----
def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def test_restatement_one_target_identity_table_is_the_contiguous_one():
    frames = _noise(6, 50, 70, 1)
    ij = np.random.default_rng(2).integers(-3, 75, (6, 2))
    want = R.Diagnose(True).render(list(frames), [tuple(p) for p in ij])
    ov = OR.Overlay(1, True)
    assert np.array_equal(ov.render(frames, np.arange(6), ij[None]), want)
    # the trace runs on across calls, as the contiguous one's does
    a, b = OR.Overlay(1, False), R.Diagnose(False)
    got = np.concatenate([a.render(frames, np.arange(0, 2), ij[None, :2]), a.render(frames, np.arange(2, 6), ij[None, 2:])])
    assert np.array_equal(got, b.render(list(frames), [tuple(p) for p in ij]))
    assert OR.Overlay(3).render(frames, [], np.zeros((3, 0, 2))).shape == (0, 360, 640)


def test_restatement_table_and_targets():
    """A table names the frame of each output; every target keeps its own trace; set_targets empties them."""
    frames = _noise(4, 40, 60, 3)
    table = [2, 2, 0, 3, 1]
    ij = np.random.default_rng(4).integers(1, 40, (2, 5, 2))
    ov = OR.Overlay(2)
    got = ov.render(frames, table, ij)
    assert [len(t) for t in ov.traces] == [5, 5] and ov.traces[0] != ov.traces[1]
    one = [OR.Overlay(1).render(frames, table, ij[t:t + 1]) for t in (0, 1)]
    plain = np.stack([R.resize(frames[f]) for f in table])
    drawn = (one[0] != plain) | (one[1] != plain)
    assert np.array_equal(got[~drawn], plain[~drawn]) and (got[drawn] == 255).all()     # the union of the two targets' pixels
    assert not np.array_equal(got, OR.Overlay(2).render(frames, table, np.stack([ij[0], ij[0]])))   # target 1 is drawn
    assert not np.array_equal(got, ov.render(frames, table, ij))                            # the traces ran on
    ov.set_targets(2)
    assert np.array_equal(got, ov.render(frames, table, ij))


# ---- the binding's own checks (host tensors: the device is looked at last) ----
def test_frame_table_and_positions_argument_checks():
    import torch
    a = _args.host_steps([0, 5, 5, 2], "frame_table")
    assert a.dtype == np.int32 and a.flags.c_contiguous and a.tolist() == [0, 5, 5, 2]
    assert _args.host_steps(np.arange(10, dtype=np.int64)[::3], "frame_table").tolist() == [0, 3, 6, 9]
    assert _args.host_steps(torch.tensor([3, 1]), "frame_table").tolist() == [3, 1]
    assert _args.host_steps([], "frame_table").shape == (0,)
    for exc, v in ((TypeError, [0.0, 1.0]), (ValueError, [[0, 1]]), (ValueError, 3), (ValueError, [2**31]), (ValueError, [-2**31 - 1])):
        with pytest.raises(exc, match="frame_table"):
            _args.host_steps(v, "frame_table")
    wide = torch.zeros((3, 20, 2), dtype=torch.int32)
    bad = [
        (TypeError, wide.long()[:, :5]), (TypeError, wide[0]), (TypeError, wide.numpy()),
        (ValueError, wide[:, :4]),                       # 4 steps where 5 are expected
        (ValueError, wide[:, ::2][:, :5]),               # steps 4 words apart
        (ValueError, torch.zeros((3, 5, 4), dtype=torch.int32)[:, :, ::2]),     # pairs 2 words apart
        (ValueError, torch.zeros((3, 5, 3), dtype=torch.int32)[:, :, :2]),
        (ValueError, torch.zeros((2, 11), dtype=torch.int32).as_strided((2, 5, 2), (11, 2, 1))),   # an odd distance between targets
        (ValueError, torch.zeros(16, dtype=torch.int32).as_strided((2, 5, 2), (6, 2, 1))),         # targets that overlap
        (ValueError, wide[:0, :5]),
    ]
    for k, (exc, t) in enumerate(bad):
        with pytest.raises(exc, match="ij") as e:
            _args.device_positions(t, "ij", 5)
        assert type(e.value) is exc, (k, e.value)
    # what the overlay accepts passes every check but the device's: a whole result, a column slice of it, one target
    for ok in (wide[:, :5], wide[:, 7:12], wide[1:2, 3:8], torch.zeros((4, 5, 2), dtype=torch.int32), wide[:1, :5]):
        with pytest.raises(TypeError, match="must live on the GPU"):
            _args.device_positions(ok, "ij", 5)


def test_diagnostic_keywords_are_checked_before_the_device():
    import torch
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for fn, f in ((pt.track_video, frames), (pt.track_clips, frames[None])):
        args = (f, 30) if fn is pt.track_video else (f,)
        with pytest.raises(TypeError, match="diagnostic"):
            fn(*args, diagnostic="overlay.mp4")
        with pytest.raises(ValueError, match="diagnostic_chunk"):
            fn(*args, diagnostic=print, diagnostic_chunk=0)
        with pytest.raises(TypeError, match="diagnostic_chunk"):
            fn(*args, diagnostic=print, diagnostic_chunk=2.5)
        with pytest.raises(TypeError, match="cuda tensor"):                  # and then the frames, as without the keyword
            fn(*args, diagnostic=print, diagnostic_chunk=7)
