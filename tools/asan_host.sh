#!/bin/bash
# AddressSanitizer + UBSan over the HOST-only entry points of the C ABI (pdog_window_tile, pdog_mode_u8,
# pdog_gaussian_taps) on a CPU box: 3000 random geometries with frame buffers of exactly the bytes a strided
# frame owns, so any read past the frame or write past the tile is caught.  (GPU-side sanitizers are not
# available on the pool.)  These entry points live in csrc/pdog_math.cpp, plain C++ without HIP: it is built alone,
# instrumented, and the harness is linked against it.  usage: tools/asan_host.sh   — a few seconds.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/pdog_asan; mkdir -p "$OUT"
B=/opt/rocm/lib/llvm/bin
$B/clang++ -O1 -g -std=c++17 -fPIC -shared -fsanitize=address,undefined -fno-omit-frame-pointer \
    -o "$OUT/libpdog_math_asan.so" "$ROOT/pawsometracker.jl_amd/csrc/pdog_math.cpp"
$B/clang -fsanitize=address,undefined -g -I "$ROOT/include" "$ROOT/tools/asan_harness.c" -o "$OUT/asan_harness" \
    -L"$OUT" -l:libpdog_math_asan.so -Wl,-rpath,"$OUT"
ASAN_OPTIONS=detect_leaks=0 "$OUT/asan_harness"
