#!/bin/bash
# AddressSanitizer + UBSan over the host arithmetic of include/pawsome_video.h (pdog_time_axis, pdog_fps_table) on a CPU
# box: csrc/pdog_math.cpp (plain C++, no HIP) is built alone, instrumented, and the stand-alone harness tools/video_harness.c
# is linked against it — like tools/asan_host.sh for the tile packer.  Nothing here is loaded into Python or touches a GPU.
# usage: tools/asan_video.sh   — a few seconds.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/pdog_asan_video; mkdir -p "$OUT"
B=/opt/rocm/lib/llvm/bin
$B/clang++ -O1 -g -std=c++17 -fPIC -shared -fsanitize=address,undefined -fno-omit-frame-pointer \
    -o "$OUT/libpdog_math_asan.so" "$ROOT/pawsometracker.jl_amd/csrc/pdog_math.cpp"
$B/clang -fsanitize=address,undefined -g -I "$ROOT/include" "$ROOT/tools/video_harness.c" -o "$OUT/video_harness" \
    -L"$OUT" -l:libpdog_math_asan.so -Wl,-rpath,"$OUT" -lm
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/video_harness"
