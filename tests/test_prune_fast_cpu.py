"""What the pre-pass's fast paths rest on (csrc/dog_prune_words.hpp), on the host: tests/prune_fast_main.cpp holds the extremes
without odd-byte masks against a byte-by-byte maximum / minimum and the row pass's pair input formed from two centred pixels
against the converted integer sum for all 256³ inputs, bit for bit.  Built with the host compiler, once plain and
once with AddressSanitizer and UBSan; the program exits non-zero on any difference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prune_fast_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_fast_path_helpers(tmp_path, flags):
    exe = tmp_path / "prune_fast"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "0 mismatches" in p.stdout
