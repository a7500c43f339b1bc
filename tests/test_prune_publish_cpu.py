"""The pre-pass's packed arrival word (csrc/dog_prune_publish.hpp) on the host: tests/prune_publish_main.cpp runs the
fetch-adds of a batch one after the other in random arrival orders, for random per-workgroup (jobs, kept pairs), and holds
what every arriver derives from the returned word against the direct sums — the list bases partition [0, Σ jobs) in arrival
order, exactly one arriver sees n − 1 arrivals, and the sums it reconstructs, the cumulative counts, the host word and the
list's header it would publish are the direct ones.  The fit test: each field at its largest fitting value (2²⁰ − 1 arrivals,
2²⁰ − 1 jobs, 2²⁴ − 1 pairs, every workgroup contributing its largest count) does not carry into its neighbour, and one past
each bound selects the fenced publish.  Built with the host compiler, once plain and once with AddressSanitizer and UBSan;
the program exits non-zero on any difference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prune_publish_main.cpp")
INC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_arrivals_in_any_order(tmp_path, flags):
    exe = tmp_path / "prune_publish"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout
