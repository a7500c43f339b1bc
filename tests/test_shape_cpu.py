"""The shape rule (include/pawsome_shape.h) as far as no GPU is needed: the header against _lib.SHAPE_PROTOTYPES and the
library's exports, the two host entry points (pdog_shape_derive, pdog_shape_headings) against the NumPy restatement on
every scene, their refusals, the Python-side argument checks, the rule's known answers and its accuracy on the restatement
alone (which the GPU must equal bit for bit: tests/test_gpu_shape.py), and the Float64 part under the host compiler in a
stand-alone program (tests/shape_rule_main.cpp, built plain and with AddressSanitizer and UBSan)."""
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
from pawsometracker_jl_amd import _args, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_restatement as SR  # noqa: E402
import shape_scenes as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "pawsome_shape.h")
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
NAMES = ["pdog_shape", "pdog_shape_derive", "pdog_shape_headings"]
P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731


# ---- the Float64 part under the host compiler ----
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_rule_program_matches_its_table(tmp_path, flags):
    exe = tmp_path / "shape_rule"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "shape_rule_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert re.search(r"\b[1-9][0-9]* checks, 0 mismatches", p.stdout)


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


def test_shape_symbols_are_declared_bound_and_exported():
    protos = _prototypes(HDR)
    assert [name for name, _ in protos] == list(_lib.SHAPE_PROTOTYPES) == list(_lib.SHAPE_SYMBOLS) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos:
        assert hasattr(L, name), name
        restype, argtypes = _lib.SHAPE_PROTOTYPES[name]
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(args) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(args, argtypes)):
            if "*" in decl or "[" in decl:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, k, decl)
            else:
                assert ctype is scalars[[w for w in decl.split() if w != "const"][0]], (name, k, decl)
    assert len(dict(protos)["pdog_shape"]) == 12
    text = open(HDR).read()
    assert "#define PDOG_SHAPE_MAX_RADIUS 127" in text and pt.SHAPE_MAX_RADIUS == _lib.SHAPE_MAX_RADIUS == SR.MAX_RADIUS == 127
    assert "library's own addition" in text and "KNOWN LIMIT" in text and "below 2^31" in text
    main = open(os.path.join(INC, "pawsome_dog.h")).read()
    assert main.index('#include "pawsome_shape.h"') > main.index('#include "pawsome_background.h"')       # at its end
    assert pt.lib().pdog_abi_version() == 1
    for fn in (pt.track_video, pt.track_frames, pt.track_segments):
        par = inspect.signature(fn).parameters
        assert par["shape"].default is False and par["shape_radius"].default is None and par["shape_min_contrast"].default is None
    par = inspect.signature(pt.BatchTracker.shapes).parameters
    assert list(par)[1:] == ["frames", "ij", "frame_index", "radius", "min_contrast", "want_sums"]
    assert par["radius"].default is None and par["min_contrast"].default == 8 and par["want_sums"].default is False
    assert hasattr(pt.Tracker, "shape") and callable(pt.shape_derive) and callable(pt.headings)


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pawsome_dog.h"\n'
                   "int use(pdog_tracker *t, const uint8_t *f, const int32_t *ij, int32_t *s, double *o, const double *th) {\n"
                   "    return pdog_shape(t, f, 0, 1, 1, 0, ij, 1, PDOG_SHAPE_MAX_RADIUS, 8, s, o) + pdog_shape_derive(s, ij, o)\n"
                   "         + pdog_shape_headings(th, ij, 1, 1.0, o);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)])
    subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)])
    for hdr in (HDR, os.path.join(INC, "pawsome_dog.h")):
        subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", hdr])
        subprocess.check_call(["g++", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", hdr])


# ---- the host entry points against the restatement ----
def _lib_derive(sums, ij):
    out = np.full(6, -7.0)
    s, p = np.ascontiguousarray(sums, np.int32), np.ascontiguousarray(ij, np.int32)
    assert pt.lib().pdog_shape_derive(P(s), P(p), P(out)) == _lib.PDOG_OK
    return out


def _clamped(c):
    return np.stack([np.clip(c.ij[:, 0], 1, SS.H), np.clip(c.ij[:, 1], 1, SS.W)], 1).astype(np.int32)


@pytest.mark.parametrize("name", [c.name for c in SS.cases()])
def test_derive_equals_the_restatement(name):
    c = SS.case(name)
    want, words = SS.reference(c)
    ij = _clamped(c)
    got = np.stack([_lib_derive(words[k], ij[k]) for k in range(len(ij))])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(want).all(axis=1), words[:, 0] == 0)          # NaN exactly where the mask is empty
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12
    assert np.array_equal(np.isnan(pt.shape_derive(words, ij)), np.isnan(want))
    assert np.abs(pt.shape_derive(words, ij)[ok] - want[ok]).max(initial=0.0) <= 1e-12
    assert pt.shape_derive(words[0], ij[0]).shape == (6,)


def test_derive_on_seeded_sums():
    """Sums of random masks in the largest disc, from every position: the int64 numerators at work."""
    rng = np.random.default_rng(5)
    dy, dx = SR.disc_offsets(127)
    for k in range(40):
        m = rng.random(len(dy)) < rng.random()
        if k == 0:
            m[:] = True
        y, x = dy[m], dx[m]
        s = np.array([m.sum(), y.sum(), x.sum(), (y * y).sum(), (y * x).sum(), (x * x).sum(), 3, 9], np.int64)
        assert np.abs(s).max() < 2**31
        ij = (int(rng.integers(1, 2000)), int(rng.integers(1, 2000)))
        want, got = SR.derive(s, ij), _lib_derive(s, ij)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.abs(got - want)[~np.isnan(want)].max(initial=0.0) <= 1e-12, (k, got, want)


def _lib_headings(theta, ij, min_step=1.0):
    th, p = np.ascontiguousarray(theta, np.float64), np.ascontiguousarray(ij, np.int32)
    out = np.full(len(th), -7.0)
    assert pt.lib().pdog_shape_headings(P(th), P(p), len(th), float(min_step), P(out)) == _lib.PDOG_OK
    return out


def _same(a, b, tol=1e-12):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.abs(a - b)[~np.isnan(b)].max(initial=0.0) <= tol


def test_headings_equal_the_restatement():
    for c in SS.cases():
        theta = SS.reference(c)[0][:, 2]
        for ms in (0.0, 1.0, 2.5):
            assert _same(_lib_headings(theta, c.ij, ms), SR.headings(theta, c.ij, ms)), (c.name, ms)
    rng = np.random.default_rng(8)
    for k in range(50):                                  # random walks with rests and NaN
        m = int(rng.integers(1, 60))
        theta = rng.uniform(-math.pi / 2, math.pi / 2, m)
        theta[rng.random(m) < 0.2] = np.nan
        ij = np.cumsum(rng.integers(-3, 4, (m, 2)) * (rng.random((m, 1)) < 0.6), axis=0).astype(np.int32) + 50
        # (steps whose displacement is perpendicular to the axis to the last bit would leave the choice to the math library's
        # sin and cos; uniform random angles against integer displacements never are)
        want = SR.headings(theta, ij, 1.0)
        assert _same(_lib_headings(theta, ij), want), k
        assert _same(pt.headings(theta, ij), want)
        shape = np.zeros((m, 6))
        shape[:, 2] = theta
        assert _same(pt.headings(shape, ij), want)
        assert _same(pt.headings(np.stack([shape, shape]), np.stack([ij, ij]))[1], want)
        ok = ~np.isnan(want)
        assert ((want[ok] > -math.pi) & (want[ok] <= math.pi)).all()


def test_headings_follow_the_motion_keep_through_the_stop_and_turn_on_the_reversal():
    c = SS.case("moving ellipse")
    shp, _ = SS.reference(c)
    hd = np.degrees(SR.headings(shp[:, 2], c.ij))
    rad = _lib_headings(shp[:, 2], c.ij)
    assert np.abs(np.degrees(rad) - hd).max() <= 1e-9
    n, s = SS.MOVE_N, SS.STOP_N
    print("headings:", np.round(hd, 2).tolist())
    fwd, stop, back = hd[1:n + 1], hd[n + 1:n + 1 + s], hd[n + 1 + s:]
    assert np.abs(fwd - SS.MOVE_DEG).max() <= 2.0                 # along the motion: the axis's own error (measured: 0.9)
    assert np.abs(stop - SS.MOVE_DEG).max() <= 2.0                # kept through the stop
    assert np.abs(back - (SS.MOVE_DEG - 180)).max() <= 2.0 and len(back) == n      # turned by pi on the reversal
    # NaN where the shape is, and the heading picks up where it was
    theta = shp[:, 2].copy()
    theta[n + 2] = np.nan
    h2 = _lib_headings(theta, c.ij)
    assert np.isnan(h2[n + 2]) and np.array_equal(np.delete(h2, n + 2), np.delete(rad, n + 2))


def test_host_entry_points_refuse():
    L = pt.lib()
    s, ij, out, th = np.zeros(8, np.int32), np.ones(2, np.int32), np.full(6, -7.0), np.zeros(3)
    assert L.pdog_shape_derive(None, P(ij), P(out)) == _lib.PDOG_E_ARG
    assert L.pdog_shape_derive(P(s), None, P(out)) == _lib.PDOG_E_ARG
    assert L.pdog_shape_derive(P(s), P(ij), None) == _lib.PDOG_E_ARG and L.pdog_last_error().startswith(b"pdog_shape_derive")
    ij3 = np.ones((3, 2), np.int32)
    for args in ((None, P(ij3), 3, 1.0, P(out)), (P(th), None, 3, 1.0, P(out)), (P(th), P(ij3), 3, 1.0, None),
                 (P(th), P(ij3), -1, 1.0, P(out)), (P(th), P(ij3), 3, -0.5, P(out)), (P(th), P(ij3), 3, float("nan"), P(out))):
        assert L.pdog_shape_headings(*args) == _lib.PDOG_E_ARG, args[2:4]
        assert L.pdog_last_error().startswith(b"pdog_shape_headings")
    assert (out == -7.0).all()
    assert L.pdog_shape_headings(None, None, 0, 1.0, None) == _lib.PDOG_OK
    # without a tracker pdog_shape has nothing to measure with — checked before any GPU call
    assert L.pdog_shape(None, P(out), 0, 0, 1, None, P(ij), 1, 0, 8, P(s), P(out)) == _lib.PDOG_E_ARG
    assert L.pdog_last_error().startswith(b"pdog_shape")


# ---- the binding's own checks (host tensors: the device is looked at last) ----
def test_python_argument_checks():
    import torch
    assert _args.shape_args(None, 8) == (0, 8) and _args.shape_args(np.int64(127), np.int32(255)) == (127, 255) and _args.shape_args(2, 1) == (2, 1)
    for exc, r in ((TypeError, 2.0), (TypeError, True), (TypeError, "9"), (ValueError, 0), (ValueError, 1), (ValueError, 128), (ValueError, -3)):
        with pytest.raises(exc, match="radius"):
            _args.shape_args(r, 8)
    for exc, mc in ((TypeError, 8.0), (TypeError, False), (TypeError, None), (ValueError, 0), (ValueError, 256), (ValueError, -1)):
        with pytest.raises(exc, match="min_contrast"):
            _args.shape_args(None, mc)
    frames = torch.zeros((4, 20, 20), dtype=torch.uint8)
    for exc, kw in ((ValueError, dict(shape_radius=5)), (ValueError, dict(shape_min_contrast=8)), (TypeError, dict(shape=1)),
                    (ValueError, dict(shape=True, shape_radius=1)), (ValueError, dict(shape=True, shape_radius=128)),
                    (TypeError, dict(shape=True, shape_radius=2.5)), (ValueError, dict(shape=True, shape_min_contrast=0)),
                    (TypeError, dict(shape=True, shape_min_contrast=1.5))):
        with pytest.raises(exc, match="shape") as e:
            pt.track_video(frames, 30, **kw)
        assert type(e.value) is exc, kw
        with pytest.raises(exc, match="shape"):
            pt.track_frames(iter(()), **kw)          # judged before the first frame is asked for
        with pytest.raises(exc, match="shape"):
            pt.track_segments([], **kw)
    with pytest.raises(TypeError, match="cuda tensor"):
        pt.track_video(frames, 30, shape=True, shape_radius=5, shape_min_contrast=3)
    with pytest.raises(ValueError, match="sums"):
        pt.shape_derive(np.zeros(7, np.int32), [1, 1])
    with pytest.raises(ValueError, match="ij"):
        pt.shape_derive(np.zeros((2, 8), np.int32), [1, 1])
    with pytest.raises(ValueError, match="indices"):
        pt.headings(np.zeros(3), np.zeros((3, 3), np.int32))
    with pytest.raises(ValueError, match="shape_or_theta"):
        pt.headings(np.zeros(4), np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match="min_step"):
        pt.headings(np.zeros(3), np.zeros((3, 2), np.int32), -1.0)
    with pytest.raises(TypeError, match="min_step"):
        pt.headings(np.zeros(3), np.zeros((3, 2), np.int32), "1")


# ---- known answers, on the restatement alone ----
@pytest.mark.parametrize("tw, n, width", [(10, 81, 10.155), (25, 441, 23.696)])
@pytest.mark.parametrize("darker", [True, False], ids=["dark", "bright"])
def test_discs_have_their_known_answers(tw, n, width, darker):
    c = SS.case(f"disc tw {tw} {'dark' if darker else 'bright'}")
    shp, words = SS.reference(c)
    assert (words[:, 0] == n).all() and (words[:, 6] == 128).all()
    assert np.abs(shp[:, 5] - width).max() < 5e-4
    assert np.abs(shp[:, 3] - shp[:, 4]).max() <= 1e-9                  # major == minor (t = hypot(0, 0) or of rounding residue)
    assert (shp[:, 0] == c.truth[0][0]).all() and (shp[:, 1] == c.truth[0][1]).all()      # the disc's centre exactly, from every position


def test_degenerate_scenes():
    for name in ("flat", "empty floor min_contrast 8", "corner disc dark fill 0"):
        shp, words = SS.reference(SS.case(name))
        assert np.isnan(shp).all() and (words[:, :6] == 0).all(), name
    shp, words = SS.reference(SS.case("empty floor min_contrast 1"))
    assert (words[:, 0] > 0).all() and (words[:, 7] < 8).all() and not np.isnan(shp).any()
    # most of the patch outside the frame: the fill is the median, the clamped positions agree with the clamping ones
    for name, b in (("corner disc dark fill 255", 255), ("corner disc bright fill 0", 0)):
        c = SS.case(name)
        shp, words = SS.reference(c)
        assert (words[:, 6] == b).all() and (words[:, 0] > 0).all() and np.array_equal(words[1], words[2]) and np.array_equal(shp[1], shp[2]), name
    # the known limit: the second object is counted at R = 25 and pulls the centroid and the axis towards it; a radius that
    # fits the animal leaves it out
    wide, w_words = SS.reference(SS.case("second object R 25"))
    fit, f_words = SS.reference(SS.case("second object R 10"))
    assert f_words[0, 0] == 113 and (fit[0, 0], fit[0, 1]) == (60.0, 80.0) and abs(fit[0, 3] - fit[0, 4]) <= 1e-9
    assert w_words[0, 0] == 113 + 29 and wide[0, 1] > 82.5 and wide[0, 3] > 2 * wide[0, 4]


# On the restatement, which the GPU equals bit for bit.  The issue's prototype measured 1.12 degrees / 0.20 px for the (12, 5)
# ellipse and 4.2 degrees for the (6, 3) one and set 2 and 6 degrees, axes within 1 px and the centroid within 0.5 px.  This
# file's generator (its noise stream, its sub-pixel centres) is not the prototype's and gives the numbers below, so, as the
# issue rules for that case, each bound is ALSO held to the restatement's worst case here plus a quarter of it — the tighter
# of the two applies.  Measured on the committed scenes, worst over the 36 angles x 3 positions (dark / bright):
#   (12, 5) R 25: angle 0.961 / 0.851 degrees, major 23.55 ... 24.43, minor 9.69 ... 10.23, centroid 0.246 / 0.168 px
#   (6, 3)  R 12: angle 3.841 / 3.841 degrees, major 11.38 ... 12.63, minor 5.44 ... 6.36, centroid 0.314 / 0.242 px
ACCURACY = {        # (a, b, R): (issue's angle bound, worst angle, worst |major - 2a|, worst |minor - 2b|, worst centroid error)
    (12, 5, 25): (2.0, 0.961, 0.45, 0.31, 0.246),
    (6, 3, 12): (6.0, 3.841, 0.63, 0.56, 0.314),
}


@pytest.mark.parametrize("key", list(ACCURACY), ids=lambda k: f"{k[0]}x{k[1]} R{k[2]}")
@pytest.mark.parametrize("tone", ["dark", "bright"])
def test_orientation_axes_and_centroid_of_drawn_ellipses(key, tone):
    a, b, R = key
    c = SS.case(f"ellipse ({a}, {b}) R {R} {tone}")
    shp, words = SS.reference(c)
    assert len(shp) == 108 and (words[:, 0] > 0).all()
    ang = max(SS.angle_error_deg(s[2], t[2]) for s, t in zip(shp, c.truth))
    cen = max(math.hypot(s[0] - t[0], s[1] - t[1]) for s, t in zip(shp, c.truth))
    dmaj, dmin = np.abs(shp[:, 3] - 2 * a).max(), np.abs(shp[:, 4] - 2 * b).max()
    print(f"{c.name}: angle {ang:.3f} deg, major {shp[:, 3].min():.2f} ... {shp[:, 3].max():.2f}, minor {shp[:, 4].min():.2f} ... "
          f"{shp[:, 4].max():.2f}, centroid {cen:.3f} px, n {words[:, 0].min()} ... {words[:, 0].max()}")
    bound, w_ang, w_maj, w_min, w_cen = ACCURACY[key]
    assert ang <= min(bound, 1.25 * w_ang)
    assert dmaj <= min(1.0, 1.25 * w_maj) and dmin <= min(1.0, 1.25 * w_min)
    assert cen <= min(0.5, 1.25 * w_cen)
    assert ((shp[:, 2] > -math.pi / 2) & (shp[:, 2] <= math.pi / 2)).all()
    assert np.abs(shp[:, 5] - 2 * math.sqrt(a * b)).max() <= 1.0             # the equivalent diameter of the ellipse's area
