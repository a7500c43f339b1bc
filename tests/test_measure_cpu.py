"""CPU-side checks of the measurement layer: the sub-pixel rule's host helper (pdog_subpixel) against the NumPy
restatement (tests/measure_restatement.py) bit for bit, its hand cases and argument checks, the restatement's responses
against the stored golden windows, and the accuracy condition on the yardstick itself (the oracle alone).  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pawsometracker_jl_amd as pt
from pawsometracker_jl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_subpixel(r5, ij):
    r = np.ascontiguousarray(r5, np.float64)
    src = (C.c_int32 * 2)(int(ij[0]), int(ij[1]))
    out = np.empty(2, np.float64)
    assert pt.lib().pdog_subpixel(r.ctypes.data, src, out.ctypes.data) == 0
    return out


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pawsome_dog.h")).read()
    declared = set(re.findall(r"\b(pdog_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("pdog_subpixel", "pdog_measure"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.pdog_abi_version() == 1                       # purely additive: the ABI version stays
    assert pt.lib().pdog_measure.argtypes is not None and pt.lib().pdog_subpixel.argtypes is not None


def test_subpixel_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    n_moved = 0
    for k in range(20000):
        kind = k % 5
        if kind == 0:            # a peak with neighbours a little below it: the usual case
            c = rng.uniform(0.01, 0.2)
            r5 = np.array([c] + list(c - rng.uniform(0, 1e-3, 4)))
        elif kind == 1:          # anything
            r5 = rng.normal(0, 1, 5)
        elif kind == 2:          # last-bit neighbours: tiny den, quotients that need the clamp
            c = rng.uniform(-1, 1)
            r5 = np.array([c] + [np.nextafter(c, -np.inf) if rng.random() < 0.5 else c - rng.uniform(0, 1e-15) for _ in range(4)])
        elif kind == 3:          # wide range of magnitudes, subnormals included
            r5 = rng.normal(0, 1, 5) * 10.0 ** rng.integers(-320, 300, 5)
        else:                    # raw bit patterns (NaN and infinities among them)
            r5 = rng.integers(0, 2 ** 64, 5, dtype=np.uint64).view(np.float64)
        ij = (int(rng.integers(-5, 2000)), int(rng.integers(-5, 2000)))
        got, ref = _c_subpixel(r5, ij), np.array(R.subpixel(r5, ij))
        same = (_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))
        assert same.all(), (r5.tolist(), ij, got.tolist(), ref.tolist())
        n_moved += int(got[0] != ij[0]) + int(got[1] != ij[1])
    assert n_moved > 10000      # the cases do exercise the division


def test_subpixel_hand_cases():
    ij = (7, 9)
    assert _c_subpixel([1.0, 0.5, 0.5, 0.25, 0.25], ij).tolist() == [7.0, 9.0]          # symmetric -> 0
    assert _c_subpixel([1.0, 1.5, 0.5, 0.0, 2.0], ij).tolist() == [7.0, 9.0]            # den == 0 -> 0
    assert _c_subpixel([1.0, 2.0, 3.0, 1.5, 1.5], ij).tolist() == [7.0, 9.0]            # den > 0 (a minimum) -> 0
    assert _c_subpixel([1.0, 1.0, 1.0, 1.0, 1.0], ij).tolist() == [7.0, 9.0]            # flat -> 0
    nan = float("nan")
    assert _c_subpixel([nan, 0.5, 0.5, 0.5, 0.5], ij).tolist() == [7.0, 9.0]            # NaN -> 0
    assert _c_subpixel([1.0, nan, 0.5, 0.5, nan], ij).tolist() == [7.0, 9.0]
    assert _c_subpixel([1.0, 1.5, 0.0, 0.0, 1.5], ij).tolist() == [6.5, 9.5]            # c=1, m=1.5, p=0 -> clamped -0.5 (and +0.5)
    assert _c_subpixel([1.0, 0.5, 0.75, 0.75, 0.5], ij).tolist() == [7.0 + 1 / 6, 9.0 - 1 / 6]   # 0.5 * (m - p) / (m + p - 2c)
    assert pt.subpixel([1.0, 0.5, 0.75, 0.75, 0.5], ij) == (7.0 + 1 / 6, 9.0 - 1 / 6)


def test_subpixel_rejects_null_pointers():
    L = pt.lib()
    r = np.ones(5)
    ij = (C.c_int32 * 2)(1, 1)
    out = np.empty(2)
    assert L.pdog_subpixel(None, ij, out.ctypes.data) == _lib.PDOG_E_ARG
    assert L.pdog_subpixel(r.ctypes.data, None, out.ctypes.data) == _lib.PDOG_E_ARG
    assert L.pdog_subpixel(r.ctypes.data, ij, None) == _lib.PDOG_E_ARG
    assert b"pdog_subpixel" in L.pdog_last_error()
    # without a tracker pdog_measure has nothing to measure with — checked before any GPU call
    assert L.pdog_measure(None, out.ctypes.data, 0, 0, 1, None, ij, 1, None, out.ctypes.data) == _lib.PDOG_E_ARG


def test_restated_peak_value_is_the_golden_maximum(oracle, golden):
    """resp5[0] at the stored position is the maximum `findmax` saw (src/PawsomeTracker.jl:59) — where the stored
    position is the window's peak itself and not its clamped image (:61)."""
    n = 0
    for c in golden:
        resp = c["resp"]
        x, y = divmod(int(np.argmax(resp.reshape(-1, order="F"))), resp.shape[0])    # findmax: first maximum, column-major
        peak = (c["guess"][0] - c["ws"][0] // 2 + y, c["guess"][1] - c["ws"][1] // 2 + x)
        if peak != c["ij"]:
            continue            # clamped into the frame: the stored position is not where the maximum sits
        K = oracle.dog_kernel(oracle.sigma(c["tw"]), c["darker"])
        r5 = R.resp5(oracle, c["frame"], c["fill"], K, c["ij"])
        assert r5[0] == resp.max(), c["name"]
        assert r5[0] == resp[y, x]
        n += 1
    assert n >= 3


@pytest.mark.parametrize("darker", [True, False])
@pytest.mark.parametrize("target_width", [25, 10])
def test_accuracy_condition_holds_for_the_oracle_alone(oracle, target_width, darker):
    """The yardstick of the GPU test: on the spiral clip the rule applied to the ORACLE's responses at the ORACLE's
    positions has less than half the RMSE of the integer positions against the true centres."""
    frames, centres = R.spiral_clip(0, darker)
    ws = pt.fix_window_size(pt.guess_window_size(target_width))
    ijs, fill, K = R.oracle_chain(oracle, frames, target_width, ws, darker)
    sub, _ = R.measure(oracle, frames, fill, K, ijs)
    e_int, e_sub = R.rmse(ijs, centres), R.rmse(sub, centres)
    print(f"spiral clip tw={target_width} darker={darker}: RMSE integer {e_int:.4f} px, sub-pixel {e_sub:.4f} px")
    assert e_int < 1.0            # it tracks (the reference's own bar: RMSE < 1 pixel)
    assert e_sub < 0.5 * e_int


def test_measure_kernel_has_no_float64_fma_and_no_scratch():
    """The built code object: dog_measure_kernel holds no v_fma_f64 (a contracted a*b + c would round once where the
    reference rounds twice), uses no scratch and spills no register."""
    B = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc", "_obj", "pawsome_dog.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(B, "llvm-objdump"))):
        pytest.skip("no object file / no LLVM tools next to this checkout (the library was built elsewhere)")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call([f"{B}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        targets = subprocess.check_output([f"{B}/clang-offload-bundler", "--list", "--type=o", f"--input={fat}"], text=True).split()
        target = [t for t in targets if "gfx950" in t][0]
        subprocess.check_call([f"{B}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={target}", f"--output={co}"])
        notes = subprocess.check_output([f"{B}/llvm-readelf", "--notes", co], text=True)
        name = re.search(r"\.name:\s+(\S*dog_measure_kernel\S*)", notes).group(1)
        isa = subprocess.check_output([f"{B}/llvm-objdump", "-d", f"--disassemble-symbols={name}", co], text=True)
    assert "v_mul_f64" in isa and "v_add_f64" in isa      # it is the kernel, and the chain is in it
    assert "v_fma_f64" not in isa
    blk = [b for b in notes.split("  - .agpr_count:")[1:] if "dog_measure_kernel" in b][0]
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1)) == 0, key
