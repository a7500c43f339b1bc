"""The run-time loader behind pdog_group_create without a GPU and without RCCL (csrc/pdog_dl.hpp), as the stand-alone program
tests/group_open_main.cpp, plain and under AddressSanitizer and UBSan.  Every machine the suite runs on has librccl, so the
branch a machine WITHOUT it takes — no name opens, the error text is built from dlerror() — ran nowhere; it read dlerror()
twice, the second call returns NULL, and the text was built from that NULL (a crash where PDOG_E_NODEV was due).  Here the
names are ones no machine has, then a library that lacks the symbols, then a library and a symbol that exist."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
MISSING = ["libpdog-no-such-library.so.1", "libpdog-no-such-library.so", "/nonexistent/lib/libpdog-no-such-library.so.1"]
RCCL_SYMBOLS = ["ncclCommInitAll", "ncclCommDestroy", "ncclGroupStart", "ncclGroupEnd", "ncclGather", "ncclGetErrorString"]


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("group_open") / "group_open_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *request.param, "-I", CSRC,
                           os.path.join(ROOT, "tests", "group_open_main.cpp"), "-o", str(exe), "-ldl"])

    def run(what, names, symbols):
        p = subprocess.run([str(exe), what, str(len(names)), *names, *symbols], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:] + p.stderr[-2000:])      # (a crash or a sanitizer's report otherwise)
        lines = p.stdout.splitlines()
        assert lines[0] in ("handle 0", "handle 1") and lines[-1].startswith("error")
        return lines[0] == "handle 1", lines[1:-1], lines[-1][len("error "):]
    return run


def test_the_loader_header_is_what_the_group_opens_rccl_with():
    """rccl() in pawsome_group.hip goes through the header under test, with its three names and six symbols, and the
    double dlerror() is gone from the tree's native code."""
    src = open(os.path.join(CSRC, "pawsome_group.hip")).read()
    assert '#include "pdog_dl.hpp"' in src and 'open_first("librccl"' in src
    assert all(f'"{s}"' in src for s in RCCL_SYMBOLS)
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp", ".cpp")) and name != "pdog_dl.hpp":      # the loader's text is read in the header alone
            assert "dlerror" not in open(os.path.join(CSRC, name)).read(), name
    hdr = open(os.path.join(CSRC, "pdog_dl.hpp")).read()
    assert set(__import__("re").findall(r"#include <([^>]+)>", hdr)) == {"dlfcn.h", "string"} and '#include "' not in hdr


def test_no_name_opens(program):
    opened, symbols, error = program("librccl", MISSING, RCCL_SYMBOLS)
    assert not opened and symbols == []
    assert error.startswith("librccl not found (") and error.endswith(")")
    reason = error[len("librccl not found ("):-1]
    assert reason and reason != "dlopen failed"                  # the loader's own text …
    assert MISSING[-1] in reason and "No such file" in reason    # … of the last failure: the name tried and why it did not open


def test_a_library_without_the_symbols(program):
    opened, symbols, error = program("librccl", MISSING[:1] + ["libm.so.6"], RCCL_SYMBOLS)
    assert opened and symbols == [f"symbol {s} 0" for s in RCCL_SYMBOLS]
    assert error == "librccl lacks ncclCommInitAll"              # the first missing symbol only


def test_a_library_and_a_symbol_that_exist(program):
    opened, symbols, error = program("libm", ["libm.so.6"], ["cos"])
    assert opened and symbols == ["symbol cos 1"] and error == ""
    opened, symbols, error = program("libm", MISSING[:2] + ["libm.so.6"], ["cos", "no_such_function_in_libm", "sin"])
    assert opened and symbols == ["symbol cos 1", "symbol no_such_function_in_libm 0", "symbol sin 1"]
    assert error == "libm lacks no_such_function_in_libm"        # an earlier failed dlopen leaves nothing behind
