"""The pre-pass's clamped loads (csrc/dog_prune_words.hpp: pw_clamp_col, pw_clamp_row, pw_shift, pw_rebuild32 / 64) on the
host: tests/prune_clamp_main.cpp rebuilds every dword and 8-byte word of small frames from the load at the clamped address —
every clamp distance to the left and to the right, rows above and below the frame, frames as narrow as one load, every mask
and fill through pw_words — and compares with the byte-by-byte statement.  Each frame row is a heap block of its own, so
under AddressSanitizer a load outside the frame's columns ends the program.  Built with the host compiler, once plain and
once with AddressSanitizer and UBSan; the program exits non-zero on any difference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prune_clamp_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_clamped_words_match_bytewise(tmp_path, flags):
    exe = tmp_path / "prune_clamp"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "0 mismatches" in p.stdout
