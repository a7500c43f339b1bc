"""The pre-pass's word arithmetic (csrc/dog_prune_words.hpp) on the host: tests/prune_words_main.cpp drives the byte masks, the
fill substitution, the moment and min / max update of one dword and Σ v² and V from the moments over bands of tiles (widths
that are no multiple of 4, ranges starting at offsets 0–3, all-0, all-255, 0/255 and never-0 tiles, every dc, the widest slot
at l = 149) and compares with the direct sums in 64-bit.  Built with the host compiler, once plain and once with
AddressSanitizer and UBSan; the program exits non-zero on any difference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prune_words_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_word_helpers_match_direct_sums(tmp_path, flags):
    exe = tmp_path / "prune_words"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "0 mismatches" in p.stdout
