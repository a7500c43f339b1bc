"""The range-end rule of the roll kernel's PRUNE instances (csrc/dog_roll_range.hpp) on the host: tests/range_end_main.cpp walks
every kept range [ba, bb) of windows of nine heights (every n1 mod 8, and the 2 l + 29 rows of tests/prune_length_scenes.py)
at every kernel length of roll_lengths.def, lists by brute force the row-tap pairs whose output y = a − t the loop emits whole
(8·ba ≤ y ≤ y_end) and holds the header to them: y_end is the last emitted row, no needed pair lies in a block below
roll_end_qlo or past a shortened prologue body's last block, roll_end_qlo is the LOWEST needed block (a rule that is merely
safe fails), and a prologue body is never entered at or past its own last block.  Built with the host compiler, once plain and
once with AddressSanitizer and UBSan; the program exits non-zero on any violation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "range_end_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_range_end_rule_matches_the_pairs_counted_one_by_one(tmp_path, flags):
    exe = tmp_path / "range_end"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout
