"""The split rule (include/pawsome_split.h) as far as no GPU is needed: the header against _lib.SPLIT_PROTOTYPES and the library's
exports, the header alone under a C and a C++ compiler, the new keywords' positions and defaults and every argument refusal of the
binding, the cell's row intervals under the host compiler in a stand-alone program (tests/split_cell_main.cpp, built plain and
with AddressSanitizer and UBSan), and the restatement (tests/split_restatement.py, which the GPU must equal bit for bit:
tests/test_gpu_split.py) — alone and with far rivals against tests/blob_restatement.py, the disjoint blobs of a set, the tie
scenes, and the ellipse scenes of tests/split_scenes.py against every animal measured alone.

The ellipse margins stand over the worst values the restatement gives on these scenes (printed by the test): the split rule's
axes within 3 px of the animal alone, theta within 4 degrees, the centroid within 1.5 px, while the blob rule is more than 5 px
off in an axis for every touching animal."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blob_restatement as BLR  # noqa: E402
import blob_scenes as BLS  # noqa: E402
import split_restatement as SPR  # noqa: E402
import split_scenes as SPS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "pawsome_split.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


# ---- the row intervals under the host compiler ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_cell_program_matches_the_per_pixel_inequality(tmp_path, flags):
    exe = tmp_path / "split_cell"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "split_cell_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"\b([1-9][0-9]*) checks, 0 mismatches", p.stdout)
    assert m and int(m.group(1)) > 10_000_000


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


def test_split_symbol_is_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.SPLIT_PROTOTYPES) == list(_lib.SPLIT_SYMBOLS) == ["pdog_blob_split"]
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.SPLIT_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    args = dict(protos)["pdog_blob_split"]
    assert len(args) == 16
    assert args[7:11] == ["int n_sets", "int n_targets", "int64_t set_stride", "int64_t target_stride"]
    # pdog_blob_split is pdog_blob with the set's four in the place of n
    blob_args = dict(_prototypes(os.path.join(INC, "pawsome_blob.h")))["pdog_blob"]
    assert args[:7] == blob_args[:7] and args[11:] == blob_args[8:]
    text = open(HDR).read()
    assert '#include "pawsome_blob.h"' in text and "n_cell" in text and "n_contact" in text and "(2R)^2" in text
    # a header of its own: neither pawsome_dog.h nor pawsome_blob.h includes it
    for other in ("pawsome_dog.h", "pawsome_blob.h"):
        assert "pawsome_split.h" not in open(os.path.join(INC, other)).read()
    assert _lib.SPLIT_MAX_TARGETS == 32 and re.search(r"#define PDOG_SPLIT_MAX_TARGETS 32\b", text)
    assert pt.lib().pdog_abi_version() == 1


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_split.h"\n'
                   "int use(pdog_tracker *t, const uint8_t *f, const int32_t *ij, int32_t *s, double *o) {\n"
                   "    return pdog_blob_split(t, f, 0, 1, 1, 0, ij, 1, PDOG_SPLIT_MAX_TARGETS, PDOG_SPLIT_MAX_TARGETS, 1, PDOG_SHAPE_MAX_RADIUS, 8, 4, s, o)\n"
                   "           + pdog_blob(t, f, 0, 1, 1, 0, ij, 1, 2, 8, 4, s, o) + pdog_shape_derive(s, ij, o);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", HDR])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", HDR])


def test_new_keywords_and_methods():
    par = inspect.signature(pt.track_video).parameters
    names = list(par)
    assert names[names.index("shape_connectivity") + 1] == "shape_split" and par["shape_split"].default is False
    assert names[names.index("shape_split") + 1] == "background"
    for fn in (pt.track_frames, pt.track_segments):                  # one target: no new keyword
        assert "shape_split" not in inspect.signature(fn).parameters
    par = inspect.signature(pt.BatchTracker.split_blobs).parameters
    assert list(par)[1:] == ["frames", "ij", "frame_index", "radius", "min_contrast", "connectivity", "targets_first", "want_sums"]
    assert par["frame_index"].default is None and par["radius"].default is None and par["min_contrast"].default == 8
    assert par["connectivity"].default == 8 and par["targets_first"].default is False and par["want_sums"].default is False


def test_python_argument_checks():
    import torch
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for exc, kw in ((ValueError, dict(shape_split=True)), (ValueError, dict(shape=True, shape_split=True)),
                    (ValueError, dict(shape_connectivity=8, shape_split=True)), (TypeError, dict(shape=True, shape_connectivity=8, shape_split=1)),
                    (TypeError, dict(shape_split=None)), (ValueError, dict(shape=True, shape_connectivity=6, shape_split=True))):
        with pytest.raises(exc, match="shape") as e:
            pt.track_video(frames, 30, **kw)
        assert type(e.value) is exc, kw
    with pytest.raises(TypeError, match="cuda tensor"):              # the keywords pass: the host frames are met next
        pt.track_video(frames, 30, shape=True, shape_connectivity=4, shape_split=True)
    # split_blobs judges everything about its arguments before it needs the device (a host tensor ends in TypeError, last)
    bt = object.__new__(pt.BatchTracker)
    bt._hw = (20, 20)
    bt.use_torch_stream = lambda: None
    ij = torch.ones((4, 3, 2), dtype=torch.int32)
    for exc, match, a, kw in ((ValueError, "connectivity", (frames, ij), dict(connectivity=6)),
                              (TypeError, "connectivity", (frames, ij), dict(connectivity=8.0)),
                              (ValueError, "radius", (frames, ij), dict(radius=1)),
                              (ValueError, "radius", (frames, ij), dict(radius=128)),
                              (ValueError, "min_contrast", (frames, ij), dict(min_contrast=0)),
                              (TypeError, "min_contrast", (frames, ij), dict(min_contrast=None)),
                              (TypeError, "targets_first", (frames, ij), dict(targets_first=1)),
                              (TypeError, "frames", (frames.float(), ij), {}),
                              (ValueError, "frames", (frames[:, :, :19], ij), {}),
                              (TypeError, "frames", (frames, ij), {}),                                  # on the host
                              ):
        with pytest.raises(exc, match=match) as e:
            bt.split_blobs(*a, **kw)
        assert type(e.value) is exc, (match, kw)
    # without a tracker pdog_blob_split has nothing to measure with — checked before any GPU call
    out, s, p = np.zeros(6), np.zeros(12, np.int32), np.ones(2, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert pt.lib().pdog_blob_split(None, P(out), 0, 0, 1, None, P(p), 1, 1, 1, 1, 0, 8, 8, P(s), P(out)) == _lib.PDOG_E_ARG
    assert pt.lib().pdog_last_error().startswith(b"pdog_blob_split")


# ---- the restatement alone ----
def _split(c, connectivity):
    return SPS.reference(c, connectivity)


def test_one_target_and_far_rivals_equal_the_blob_rule():
    seen = 0
    for c in list(BLS.cases()) + [g[k] for _, g in BLS.noise_cases() for k in (3, 23, 60)]:
        for connectivity in c.conns:
            want = BLS.reference(c, connectivity)[1]
            R = c.radius
            h, w = c.frames.shape[1:]
            for k, p in enumerate(c.ij):
                one = SPR.sums_at(c.frames[c.fi[k]], [p], 0, R, c.fill, c.darker, c.min_contrast, connectivity)[0]
                assert np.array_equal(one[:10], want[k]) and one[10] == want[k][8] and one[11] == 0, (c.name, k)
                i, j = SPR.clamp(p, h, w)
                far = [(i, j + 2 * R + 1) if j + 2 * R + 1 <= w else (i, j - 2 * R - 1), p, (i + 2 * R + 1, j) if i + 2 * R + 1 <= h else (i - 2 * R - 1, j)]
                if all(1 <= q[0] <= h and 1 <= q[1] <= w for q in far):         # (clamping would bring them nearer)
                    got = SPR.sums_at(c.frames[c.fi[k]], far, 1, R, c.fill, c.darker, c.min_contrast, connectivity)[0]
                    assert np.array_equal(got, one), (c.name, k)
                    seen += 1
    assert seen >= 20


def _frame_pixels(c, connectivity):
    """Per target of set 0 the blob's pixels as a set of frame coordinates."""
    out = []
    for a in range(c.ij.shape[1]):
        blob, _, _, _, _, _, p = SPR.parts_at(c.frames[0], c.ij[0], a, c.radius, c.fill, c.darker, c.min_contrast, connectivity)
        ys, xs = np.nonzero(blob)
        out.append({(int(p[0] + y - c.radius), int(p[1] + x - c.radius)) for y, x in zip(ys, xs)})
    return out


def test_blobs_of_one_set_never_share_a_frame_pixel():
    nonempty = 0
    for name in ("side by side", "T", "three", "same pixel", "bisector ties", "rival at 2R", "32 targets", "tier R 32", "overhang fill 40"):
        c = SPS.case(name)
        for connectivity in c.conns:
            px = _frame_pixels(c, connectivity)
            nonempty += sum(bool(s) for s in px)
            for a in range(len(px)):
                for b in range(a + 1, len(px)):
                    assert not (px[a] & px[b]), (name, connectivity, a, b)
    assert nonempty > 60


def test_tie_scenes():
    for connectivity in (4, 8):
        # a lower-index rival on the same pixel: nothing left, the contrast and the mask are there
        w = _split(SPS.case("same pixel"), connectivity)[1][0]
        assert w[0, 0] > 0 and w[0, 11] == 0 and w[0, 10] == w[0, 8]          # target 0 wins every tie: the whole mask
        assert w[1, 0] == 0 and w[1, 10] == 0 and w[1, 7] >= 8 and w[1, 8] > 0 and w[1, 9] == 0 and w[1, 11] == 0
        assert np.isnan(_split(SPS.case("same pixel"), connectivity)[0][0, 1]).all()
        # tie pixels on both bisectors go to the lower index: every mask pixel of the union is in exactly one cell
        c = SPS.case("bisector ties")
        px = _frame_pixels(c, connectivity)
        w = _split(c, connectivity)[1][0]
        assert (w[:, 0] > 0).all() and (w[:, 11] > 0).all()
        assert (58, 79) in px[0] and (58, 79) not in px[1]                       # |x - p0| = |x - p1| = 3 on the row of both
        assert (60, 78) in px[0] and (60, 78) not in px[2]                       # 8 = 8: p0 = (58, 76), p2 = (62, 80)
        sq = {(y, x) for y in range(46, 76) for x in range(66, 96)}              # the dark square, 1-based
        union = px[0] | px[1] | px[2]
        assert union <= sq and len(union) == len(px[0]) + len(px[1]) + len(px[2])
        near = {q for q in sq if min((q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2 for p in c.ij[0]) <= 100}
        assert near <= union                                                     # nothing near the positions is lost
        # a rival at exactly 2R decides one pixel, the tie at R from both; at 2R + 1 none
        at, past = _split(SPS.case("rival at 2R"), connectivity)[1][0], _split(SPS.case("rival at 2R + 1"), connectivity)[1][0]
        blob = BLR.blobs(SPS.case("rival at 2R").frames, SPS.case("rival at 2R").ij[0], [0, 0], 12, 128, True, 8, connectivity)[1]
        assert np.array_equal(at[0, :10], blob[0]) and at[0, 10] == at[0, 8] and at[0, 11] == 0       # it keeps the tie pixel: its whole patch is its cell
        assert at[1, 10] == at[1, 8] - 1 and at[1, 0] == blob[1, 0] - 1 and at[1, 11] == 1 and at[1, 9] == blob[1, 9] - 1
        blob = BLR.blobs(SPS.case("rival at 2R + 1").frames, SPS.case("rival at 2R + 1").ij[0], [0, 0], 12, 128, True, 8, connectivity)[1]
        assert np.array_equal(past[:, :10], blob) and (past[:, 10] == past[:, 8]).all() and (past[:, 11] == 0).all()


def _angle_deg(a, b):
    d = abs(math.degrees(a - b)) % 180.0
    return min(d, 180.0 - d)


def test_ellipse_scenes_measure_every_animal_as_if_alone():
    worst = dict(axis=0.0, theta=0.0, centre=0.0)
    for name, animals in SPS.ELLIPSES.items():
        c = SPS.case(name)
        shp, words = _split(c, 8)
        merged = BLR.blobs(c.frames, c.ij[0], np.zeros(len(animals), np.int32), SPS.R_ELL, 128, True, 8, 8)
        for k in range(len(animals)):
            f, p = SPS.alone(name, k)
            one, one_w = BLR.blobs(f[None], [p], None, SPS.R_ELL, 128, True, 8, 8)
            line = f"{name} [{k}] alone / blob rule / split rule: theta {math.degrees(one[0, 2]):.1f} / {math.degrees(merged[0][k, 2]):.1f} / " \
                   f"{math.degrees(shp[0, k, 2]):.1f}, major {one[0, 3]:.2f} / {merged[0][k, 3]:.2f} / {shp[0, k, 3]:.2f}, minor {one[0, 4]:.2f} / " \
                   f"{merged[0][k, 4]:.2f} / {shp[0, k, 4]:.2f}, n_contact {words[0, k, 11]}"
            print(line)
            if k in SPS.TOUCHING[name]:
                # the blob rule is more than 5 px off in an axis, the split rule stays with the animal alone
                assert max(abs(merged[0][k, 3] - one[0, 3]), abs(merged[0][k, 4] - one[0, 4])) > 5.0, line
                d_axis = max(abs(shp[0, k, 3] - one[0, 3]), abs(shp[0, k, 4] - one[0, 4]))
                d_theta = _angle_deg(shp[0, k, 2], one[0, 2])
                d_centre = math.hypot(shp[0, k, 0] - one[0, 0], shp[0, k, 1] - one[0, 1])
                assert d_axis <= 3.0 and d_theta <= 4.0 and d_centre <= 1.5, line
                worst = dict(axis=max(worst["axis"], d_axis), theta=max(worst["theta"], d_theta), centre=max(worst["centre"], d_centre))
                assert words[0, k, 11] > 0, line
            else:
                # apart, and the third animal of three: the blob rule's measurement on the same frame, bit for bit
                assert np.array_equal(words[0, k, :10], merged[1][k]) and words[0, k, 11] == 0, line
                assert (words[0, k, 10] == words[0, k, 8]) == (name == "apart"), line      # (three: the pair lies in the third's patch)
                assert np.array_equal(shp[0, k].view(np.int64), merged[0][k].view(np.int64)), line
    print("worst over the touching animals:", worst)
    assert 0.0 < worst["axis"] <= 3.0


def test_every_case_is_a_call_the_library_accepts():
    names = [c.name for c in SPS.cases()]
    assert len(set(names)) == len(names) == 17
    for c in SPS.cases():
        assert c.ij.dtype == np.int32 and c.ij.ndim == 3 and 1 <= c.ij.shape[1] <= 32 and c.ij.shape[0] <= len(c.frames)
    assert SPS.case("32 targets").ij.shape[1] == 32 and SPS.case("stack").ij.shape[:2] == (4, 2)
    for connectivity in (4, 8):
        cs = SPS.radius_cases(connectivity)
        assert [c.radius for c in cs] == list(range(2, 128)) and all(c.ij.shape == (1, 3, 2) for c in cs)
    w = _split(SPS.case("overhang fill 40"), 8)[1][0]
    assert (w[[0, 2], 8] > 0).all() and (w[[0, 2], 0] > 0).all()      # (the clamped rival's own patch is mostly padding)
    w = _split(SPS.case("bright side by side"), 8)[1][0]
    assert (w[:, 0] > 40).all() and (w[:, 11] > 0).all()
