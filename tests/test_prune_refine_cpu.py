"""The pre-pass's second stage (csrc/dog_prune.hpp, "the cell bound") stated in NumPy (tests/prune_refine_restatement.py, on top
of the unchanged first stage of tests/prune_restatement.py) and held against the response maps on the scenes of
tests/prune_refine_scenes.py — l = 17, 65 and 109, one strip, two strips with a remainder column, a shifted second strip,
windows over the frame's corner, a disc on the strips' boundary, two equal discs in different strips, bright targets, ±3 and ±40
levels of noise, flat and noise-only windows.  For every scene:
  * the refined range of every slot lies inside the first stage's;
  * every pixel outside the refined ranges has a response below L − 2δ(V) − T_max, in the FP32 map of the roll order
    (tests/fp32_restatement.py) and in the dense Float64 oracle's map;
  * the pixel that gives the window's maximum lies inside;
  * every evaluated cell bound, in the response's units, is at least the largest |response| of its 8 × 8 outputs;
  * with a target and at most ±3 levels the refined (slot, sub-chunk) pairs are strictly fewer than the first stage's; flat and
    noise-only windows keep the first stage's ranges.
Also the host's weights in a stand-alone program (tests/refine_weights_main.cpp, plain and with AddressSanitizer and UBSan),
the restatement's weights against the box sums of the dense kernel, and include/pawsome_refine.h against its prototype table.
No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_restatement as fr  # noqa: E402
import prune_restatement as pr  # noqa: E402
import prune_refine_restatement as rr  # noqa: E402
import prune_refine_scenes as scenes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
SETS = scenes.sets()


@pytest.mark.parametrize("st", SETS, ids=[s.name for s in SETS])
def test_refined_ranges_keep_what_matters(oracle, st):
    l, (n1, n2) = st.l, st.ws
    K = oracle.dog_kernel(oracle.sigma(st.tw), st.darker)
    assert oracle.kernel_len(oracle.sigma(st.tw)) == l and pr.span(l) == {17: 3, 65: 9, 109: 15}[l]
    for sc, (tile, pp, rf) in zip(st.scenes, st.stages()):
        what = (st.name, sc.name)
        resp32 = fr.response_f32(tile, st.fill, st.tw, st.darker, "roll").astype(np.float64)
        _, resp64 = oracle.detect(sc.frame, st.fill, K, st.radii, sc.guess, want_resp=True)
        resp64 = np.asarray(resp64)
        assert resp32.shape == resp64.shape == (n1, n2)
        assert np.abs(resp32 - resp64).max() <= pp["dV"] + 1e-12, what   # (the two maps within δ(V) of each other: the same window; 1e-12: the dense Float64 sum over a flat window is not exactly 0)
        inside = np.zeros((n1, n2), bool)
        for (c0, w), (ba, bb), (ra, rb) in zip(pp["slots"], pp["hull"], rf["hull"]):
            assert (ra, rb) == (0, 0) or (ba <= ra < rb <= bb), (what, (ba, bb), (ra, rb))
            inside[8 * ra:8 * rb, c0:c0 + w] = True
        thr = pp["L"] - 2.0 * pp["dV"] - pp["Tmax"]
        kept1, total = pr.kept_pairs(pp, l)
        kept2 = rr.kept_pairs(rf["hull"], l, pp["nsub"])
        print(f"{st.name} {sc.name}: first stage {pp['hull']}, second {rf['hull']}; pairs {kept1} -> {kept2} of {total}")
        for resp in (resp32, resp64):
            my, mx = np.unravel_index(int(np.argmax(resp)), resp.shape)
            assert inside[my, mx], (what, (int(my), int(mx)))
            if (~inside).any():
                assert resp[~inside].max() < thr, (what, float(resp[~inside].max()), thr)
                assert resp[~inside].max() < float(resp.max()) - pp["Tmax"], what
        unit = pp["norm"] / (255.0 * 65536.0)                        # Σ Wq·r in the response's units
        for (j, xb), B in rf["B"].items():
            block = np.abs(resp64[8 * j:8 * j + 8, 8 * xb:8 * xb + 8])
            assert B * unit + 1e-12 >= block.max(), (what, j, xb, B * unit, float(block.max()))
        if rf["tq"] is None:
            assert rf["hull"] == pp["hull"]
        if sc.quiet:
            assert kept2 < kept1, (what, kept1, kept2)
        if not sc.target:
            assert kept2 == kept1 == total and rf["hull"] == pp["hull"], (what, kept1, kept2, total)
        if sc.name == "two-discs":                                   # each disc's strip keeps its rows
            for (y, x) in st.two:
                s = [i for i, (c0, w) in enumerate(pp["slots"]) if c0 <= x < c0 + w and w > 1]
                assert any(rf["hull"][i][0] <= y // 8 < rf["hull"][i][1] for i in s), (what, y, x, rf["hull"])


def test_scene_sets_hold_what_they_claim():
    names = {s.name: s for s in SETS}
    assert names["l17-one-strip"].ws[0] % 8 and names["l65-one-strip"].ws[0] % 8
    assert len(pr.slots(45)) == 1 and pr.slots(129) == [(0, 64), (64, 64), (128, 1)] and pr.slots(101) == [(0, 64), (37, 64)]
    for st in SETS:
        assert st.nstrips() == len([1 for _, w in pr.slots(st.ws[1]) if w > 1])
        assert len(st.jobs(True)) <= len(st.jobs(False)) and st.jobs(True) != st.jobs(False), st.name


@pytest.mark.parametrize("tw", (6, 25, 44))
def test_restated_weights_bound_every_box(tw):
    gp, gm, _, _ = fr.tap_tables(tw, True)
    l, NS, norm = len(gp), pr.span(len(gp)), pr.kernel_norm_up(gp, gm)
    K2 = (np.outer(gp, gp) - np.outer(gm, gm)) ** 2
    Wq = rr.weights(gp, gm)
    for i in range(8):
        for j in range(8):
            total = 0.0
            for dy in range(NS):
                for dx in range(NS):
                    box = K2[max(8 * dy - i, 0):max(min(8 * dy - i + 8, l), 0), max(8 * dx - j, 0):max(min(8 * dx - j + 8, l), 0)].sum()
                    total += box
                    assert Wq[dy][dx] * norm / 4096.0 >= np.sqrt(box), (tw, dy, dx, i, j)
            assert abs(total - K2.sum()) <= 1e-12 * K2.sum()
    assert max(max(r) for r in Wq) <= 4097


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_host_weights_program(tmp_path, flags):
    exe = tmp_path / "refine_weights"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "refine_weights_main.cpp"), os.path.join(CSRC, "pdog_math.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert re.search(r"\b[1-9][0-9]* checks, 0 mismatches", p.stdout)


def test_prototype_table_matches_the_header():
    """include/pawsome_refine.h against _lib.REFINE_PROTOTYPES, and the library exports every name."""
    import pawsometracker_jl_amd as pt
    from pawsometracker_jl_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pawsome_refine.h")).read(), flags=re.S)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"int\s+(pdog_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)]
    assert [n for n, _ in found] == list(_lib.REFINE_PROTOTYPES) == list(_lib.REFINE_SYMBOLS) and len(found) == 1
    for name, args in found:
        restype, argtypes = _lib.REFINE_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(args.split(","))
        for ctype, decl in zip(argtypes, args.split(",")):
            assert ("*" in decl and (ctype is C.c_void_p or issubclass(ctype, C._Pointer))) or (decl.split()[0] == "int" and ctype is C.c_int), (name, decl)
        fn = getattr(pt.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert '#include "pawsome_refine.h"' in open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
    assert "no_refine" in open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
