"""The two adaptive policies of the roll batch path (csrc/pdog_policy.hpp) and the mailbox layout they read through
(csrc/pdog_mailbox.hpp) on the host: tests/policy_main.cpp states both rules a second time over 64-bit counts and compares call
by call, over fixed publication sequences (thresholds on either side, the calm count and its restart, counts that cross 2^32
between two looks, one look that covers three batches, the exact number of dense batches before a probe, waking while asleep)
and seeded random ones.  Built with the host compiler, once plain and once with AddressSanitizer and UBSan; the program exits
non-zero on any difference.  Including the mailbox header compiles its layout asserts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "policy_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_policies_match_restated_rules(tmp_path, flags):
    exe = tmp_path / "policy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout


def test_policy_header_compiles_alone(tmp_path):
    """No HIP include: the host compiler takes the header by itself, warnings as errors."""
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "pdog_policy.hpp"\nint main() { return pdog::MapPolicy().on() ? 1 : 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, str(tu), "-o", str(tmp_path / "alone")])
