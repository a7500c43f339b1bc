"""The tracker's plan (csrc/pdog_plan.hpp) on the host: tests/plan_main.cpp replays the trackers and call sequences of
tests/dispatch_cases.py through make_plan / path_for_batch / exact_thresholds, and every snapshot must equal the
characterisation recording tests/golden/dispatch_paths.json exactly — the same file tests/test_gpu_dispatch.py holds a tracker
on the GPU to, thresholds as the doubles recorded.  The recording comes from a library older than pdog_plan.hpp and is not
re-recorded.

One answer in the recording is the device's and is RESTATED here, not computed: the tracker 9801x45_l29 is refused at
creation ([[2]], PDOG_E_HIP) because hipFuncSetAttribute refuses the finishing kernel a dynamic-LDS limit beyond the CU's
LDS.  plan_main.cpp states that as "a dynamic-LDS request of the plan exceeds kMaxLds" and prints status 2 then.

The same program, mode `check`: chain_path against a second statement of its rule over a grid of clip and step counts, table
and progress, pinned and unpinned plans and resident counts; tiled_serves on either side of n · ns1 · ns2 = resident; what
Plan::part_slots has to hold; and the sub-window counts plan_tiled's comment names.  Built with the host compiler (g++ gives
the recorded threshold bits; the Makefile's compiler for pdog_math.cpp was not needed), once plain and once with
AddressSanitizer and UBSan; both new headers also compile alone, warnings as errors."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dispatch_cases import BATCHES, CASES, SEQUENCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "plan_main.cpp"), os.path.join(INC, "pdog_math.cpp")]
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_paths.json")
BUILDS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    # (-Wno-unknown-pragmas: pdog_math.cpp pins contraction with a clang pragma; the generic x86-64 target has no FMA to contract to)
    out = tmp_path_factory.mktemp("plan_" + request.param) / "plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *BUILDS[request.param], "-I", INC, *SRC, "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def recording():
    with open(FIXTURE) as f:
        doc = json.load(f)
    assert doc["batches"] == BATCHES and sorted(doc["cases"]) == sorted(CASES)
    assert all(sorted(seqs) == sorted(SEQUENCES) for seqs in doc["cases"].values())
    return doc["cases"]


def _geometry(case):
    fh, fw, tw, (wh, ww) = CASES[case]
    return [str(fh), str(fw), repr(float(tw)), str(wh), str(ww)]


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("case", sorted(CASES))
def test_replayed_plan_equals_the_recording(exe, recording, case):
    for name, calls in SEQUENCES.items():
        words = ["v:%d" % c[1] if c[0] == "set_variant" else "t:%s:%d" % (c[1], c[2]) for c in calls]
        out = _run(exe, "replay", *_geometry(case), ",".join(map(str, BATCHES)), *words)
        got = [json.loads(line) for line in out.splitlines()]
        assert got == recording[case][name], (case, name)


@pytest.mark.parametrize("case", sorted(CASES))
def test_chain_path_tiled_serves_and_part_slots(exe, case):
    out = _run(exe, "check", *_geometry(case))
    print(out)
    assert " 0 mismatches" in out and not out.startswith("0 checks")


@pytest.mark.parametrize("header", ["dog_layout.hpp", "pdog_plan.hpp"])
def test_header_compiles_alone(tmp_path, header):
    """No HIP include: the host compiler takes the header by itself, warnings as errors."""
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "%s"\nint main() { return pdog::round_up(3, 4) == 4 ? 0 : 1; }\n' % header)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, str(tu), "-o", str(tmp_path / "alone")])
