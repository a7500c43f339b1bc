"""The blob rule (include/pawsome_blob.h) as far as no GPU is needed: the header against _lib.BLOB_PROTOTYPES and the library's
exports, the header alone under a C and a C++ compiler, the new keywords' defaults and the binding's argument checks, the fill's
row-word operations under the host compiler in a stand-alone program (tests/blob_fill_main.cpp, built plain and with
AddressSanitizer and UBSan), and the restatement (tests/blob_restatement.py, which the GPU must equal bit for bit:
tests/test_gpu_blob.py) — against scipy.ndimage.label on every scene, against the shape rule's restatement where the mask is one
component, and on what every scene of tests/blob_scenes.py claims to contain."""
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
import blob_restatement as BLR  # noqa: E402
import blob_scenes as BLS  # noqa: E402
import shape_restatement as SR  # noqa: E402
import shape_scenes as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "pawsome_blob.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
DIFFERENT = {"second object R 25", "empty floor min_contrast 1"}       # the shape scenes whose mask is more than one component


# ---- the row-word operations under the host compiler ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_fill_program_matches_the_pixel_flood_fill(tmp_path, flags):
    exe = tmp_path / "blob_fill"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "blob_fill_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert re.search(r"\b[1-9][0-9]* checks, 0 mismatches", p.stdout)
    # the sweep counts DESIGN.md quotes for the filled discs: one row further per sweep, and the sweep that finds nothing
    assert "filled disc R 25: 26, R 127: 128" in p.stdout


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


def test_blob_symbol_is_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.BLOB_PROTOTYPES) == list(_lib.BLOB_SYMBOLS) == ["pdog_blob"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.BLOB_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    args = dict(protos)["pdog_blob"]
    assert len(args) == 13 and args[10] == "int connectivity"
    # pdog_blob is pdog_shape with the connectivity put in front of the outputs
    shape_args = dict(_prototypes(os.path.join(INC, "pawsome_shape.h")))["pdog_shape"]
    assert args[:10] == shape_args[:10] and args[11:] == shape_args[10:]
    text = open(HDR).read()
    assert '#include "pawsome_dog.h"' in text and "lifts the KNOWN LIMIT" in text and "TOUCH" in text and "n_mask" in text and "n_rim" in text
    # a header of its own: pawsome_dog.h stays as it is and does not include it
    assert "pawsome_blob.h" not in open(os.path.join(INC, "pawsome_dog.h")).read()
    assert pt.lib().pdog_abi_version() == 1


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_blob.h"\n'
                   "int use(pdog_tracker *t, const uint8_t *f, const int32_t *ij, int32_t *s, double *o) {\n"
                   "    return pdog_blob(t, f, 0, 1, 1, 0, ij, 1, PDOG_SHAPE_MAX_RADIUS, 8, 4, s, o) + pdog_shape_derive(s, ij, o);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", HDR])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", HDR])


def test_new_keywords_and_methods():
    for fn in (pt.track_frames, pt.track_segments):
        par = inspect.signature(fn).parameters
        assert list(par)[-1] == "shape_connectivity" and par["shape_connectivity"].default is None       # at the end
    # track_video's last five keywords are pinned by tests/test_motion_cpu.py: there it follows its siblings
    par = inspect.signature(pt.track_video).parameters
    assert list(par)[list(par).index("shape"):][:4] == ["shape", "shape_radius", "shape_min_contrast", "shape_connectivity"]
    assert par["shape_connectivity"].default is None
    par = inspect.signature(pt.BatchTracker.blobs).parameters
    assert list(par)[1:] == ["frames", "ij", "frame_index", "radius", "min_contrast", "connectivity", "want_sums"]
    assert par["radius"].default is None and par["min_contrast"].default == 8 and par["connectivity"].default == 8
    assert par["want_sums"].default is False
    par = inspect.signature(pt.Tracker.blob).parameters
    assert list(par)[1:] == ["ij", "radius", "min_contrast", "connectivity", "want_sums"] and par["connectivity"].default == 8


def test_python_argument_checks():
    import torch
    assert _args.blob_args(None, 8, 8) == (0, 8, 8) and _args.blob_args(np.int64(127), np.int32(255), np.int32(4)) == (127, 255, 4)
    for exc, k in ((TypeError, 8.0), (TypeError, True), (TypeError, "8"), (TypeError, None), (ValueError, 0), (ValueError, 6), (ValueError, -8)):
        with pytest.raises(exc, match="connectivity"):
            _args.blob_args(None, 8, k)
    with pytest.raises(ValueError, match="radius"):
        _args.blob_args(1, 8, 8)
    with pytest.raises(ValueError, match="min_contrast"):
        _args.blob_args(None, 0, 8)
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for exc, kw in ((ValueError, dict(shape_connectivity=8)), (ValueError, dict(shape=True, shape_connectivity=6)),
                    (TypeError, dict(shape=True, shape_connectivity=8.0)), (ValueError, dict(shape=True, shape_connectivity=4, shape_radius=1))):
        with pytest.raises(exc, match="shape") as e:
            pt.track_video(frames, 30, **kw)
        assert type(e.value) is exc, kw
        with pytest.raises(exc, match="shape"):
            pt.track_frames(iter(()), **kw)          # judged before the first frame is asked for
        with pytest.raises(exc, match="shape"):
            pt.track_segments([], **kw)
    with pytest.raises(TypeError, match="cuda tensor"):
        pt.track_video(frames, 30, shape=True, shape_connectivity=4)
    # without a tracker pdog_blob has nothing to measure with — checked before any GPU call
    out, s, ij = np.zeros(6), np.zeros(10, np.int32), np.ones(2, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert pt.lib().pdog_blob(None, P(out), 0, 0, 1, None, P(ij), 1, 0, 8, 8, P(s), P(out)) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_last_error().startswith(b"pdog_blob")
    # shape_derive keeps working on the first eight integers
    words = BLS.reference(BLS.case("diagonal touch"), 8)[1]
    assert np.array_equal(pt.shape_derive(words[..., :8], [[59, 79]]), BLS.reference(BLS.case("diagonal touch"), 8)[0])


# ---- the restatement against scipy.ndimage.label ----
def _label_blob(mask, seed, connectivity):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)       # the cross, or the full 3 x 3
    lab, _ = ndimage.label(mask, structure=structure)
    return (lab == lab[seed]) & mask if mask[seed] else np.zeros_like(mask)


def _all_cases():
    return list(SS.cases()) + list(BLS.cases()) + [c for _, group in BLS.noise_cases() for c in group[::9]]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_scipy_label_at_the_seed(connectivity):
    seen = 0
    for c in _all_cases():
        R = c.radius or SR.default_radius(c.tw)
        for k, p in enumerate(c.ij):
            mask, disc, seed, b, cc, _ = BLR.mask_at(c.frames[c.fi[k]], p, R, c.fill, c.darker, c.min_contrast)
            assert not mask.any() or mask[seed], (c.name, k)                      # the seed lies inside the mask
            assert disc[seed] and abs(seed[0] - R) <= 1 and abs(seed[1] - R) <= 1
            got = BLR.flood(mask, seed, connectivity)
            assert np.array_equal(got, _label_blob(mask, seed, connectivity)), (c.name, k)
            seen += int(got.any())
    assert seen > 300


# ---- where the blob is the mask, and where it is not ----
def test_blob_differs_from_the_mask_in_exactly_two_shape_scenes():
    assert len(SS.cases()) == 17
    for c in SS.cases():
        words = SS.reference(c)[1]
        for connectivity in (4, 8):
            got = BLS.reference(c, connectivity)[1]
            assert np.array_equal(got[:, 6:8], words[:, 6:8]) and np.array_equal(got[:, 8], words[:, 0]), c.name      # b, c; n_mask
            same = np.array_equal(got[:, :8], words)
            assert same == (c.name not in DIFFERENT), (c.name, connectivity)
            assert same == bool((got[:, 0] == got[:, 8]).all()), c.name
    # the noise mask of the empty floor at its last position, (30, 20)
    c = SS.case("empty floor min_contrast 1")
    assert SS.reference(c)[1][1, 0] == 174 and BLS.reference(c, 8)[1][1, 0] == 153 and BLS.reference(c, 4)[1][1, 0] == 4


def test_the_second_object_is_left_out():
    c = SS.case("second object R 25")
    for connectivity in (4, 8):
        shp, words = BLS.reference(c, connectivity)
        assert words[0, 0] == 113 and words[0, 8] == 142 and words[0, 9] == 0
        assert (shp[0, 0], shp[0, 1]) == (60.0, 80.0)
        assert shp[0, 3] == shp[0, 4]
        fit = SS.reference(SS.case("second object R 10"))[1]
        assert np.array_equal(words[0, :6], fit[0, :6])                # what the fitting radius measured


# ---- every scene contains what its name claims ----
def test_scenes_contain_what_they_claim():
    ref = lambda name, k: BLS.reference(BLS.case(name), k)[1][0]  # noqa: E731
    assert ref("diagonal touch", 8)[0] == 50 and ref("diagonal touch", 4)[0] == 25 and ref("diagonal touch", 4)[8] == 50
    # the seed tie: the (-1, -1) blob of 25 pixels, not the (+1, +1) blob of 49; the centre is at background
    c = BLS.case("seed tie")
    i, j = c.ij[0]
    f = c.frames[0]
    assert f[i - 1, j - 1] == BLS.FLOOR and f[i - 2, j - 2] == f[i, j] == BLS.DARK
    mask, _, seed, _, _, _ = BLR.mask_at(f, c.ij[0], c.radius, c.fill, True, 8)
    assert seed == (c.radius - 1, c.radius - 1)
    for k in (4, 8):
        w = ref("seed tie", k)
        assert w[0] == 25 and w[8] == 25 + 49 and w[1] < 0 and w[2] < 0          # up and to the left
        assert BLR.flood(mask, (c.radius + 1, c.radius + 1), k).sum() == 49
    assert ref("bar", 8)[9] > 0 and ref("bar", 4)[9] == ref("bar", 8)[9] == 10 and ref("bar", 8)[0] == ref("bar", 8)[8]
    # the long geodesics: one component that is the whole mask, and a long way round — the corridor's pixels against the
    # straight distance R
    for R in BLS.GEODESIC_RADII:
        for kind in ("vertical comb", "horizontal comb", "spiral"):
            w = ref(f"{kind} R {R}", 4)
            assert w[0] == w[8] > 6 * R and w[9] == 0, (kind, R)
            assert np.array_equal(w, ref(f"{kind} R {R}", 8))
    # the noise: blobs that are not the mask, that reach the rim, and, under fill 40, that run outside the frame
    groups = dict(BLS.noise_cases())
    assert all(len(g) == 126 and [c.radius for c in g] == list(range(2, 128)) for g in groups.values())
    for name, least in (("inside 0.42", 100), ("overhang 0.42 fill 128", 100), ("overhang 0.42 fill 40", 60), ("overhang 0.60 fill 128", 30)):
        w = np.stack([BLS.reference(c, c.conns[0])[1][0] for c in groups[name]])
        assert ((w[:, 0] > 0) & (w[:, 0] < w[:, 8])).sum() >= least, name
    # at density 0.60 the dark pixels are the majority of a patch inside the frame: the median is dark and the mask empty
    w = np.stack([BLS.reference(c, 4)[1][0] for c in groups["inside 0.60"]])
    assert (w[:, [0, 8, 9]] == 0).all() and (w[:, 6] == BLS.DARK).all() and (w[:, 7] == 0).all()
    outside = 0
    for c in groups["overhang 0.42 fill 40"][::5]:
        mask, _, seed, _, _, (i, j) = BLR.mask_at(c.frames[0], c.ij[0], c.radius, c.fill, True, 8)
        blob = BLR.flood(mask, seed, 8)
        rows = i - 1 - c.radius + np.arange(2 * c.radius + 1)
        outside += int(blob[(rows < 0) | (rows >= BLS.H)].any())
    assert outside >= 8
    # the two connectivities differ on the noise
    c = groups["inside 0.42"][40]
    assert BLS.reference(c, 4)[1][0, 0] < BLS.reference(c, 8)[1][0, 0]
