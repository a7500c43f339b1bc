#!/bin/bash
# usage: tools/kernel_isa.sh <object-or-so> <kernel-name-filter> [opcode-regex]  — opcode histogram of one gfx950 kernel's ISA
# (with an opcode regex: only the matching opcodes, and "0 <regex>" when none matches: `… dog_measure v_fma_f64`)
F=$1; PAT=$2; OP=${3:-}
TMP=$(mktemp -d)
B=/opt/rocm/lib/llvm/bin
$B/llvm-objcopy --dump-section .hip_fatbin=$TMP/fat.bin $F $TMP/copy.o 2>/dev/null
T=$($B/clang-offload-bundler --list --type=o --input=$TMP/fat.bin 2>/dev/null | grep gfx950 | head -1)
[ -n "$T" ] && $B/clang-offload-bundler --unbundle --type=o --input=$TMP/fat.bin --targets=$T --output=$TMP/dev.co 2>/dev/null
[ -s $TMP/dev.co ] || { echo "no gfx950 bundle in $F"; exit 1; }
SYM=$($B/llvm-readelf --notes $TMP/dev.co | sed -n 's/^ *\.name: *//p' | grep -E "$PAT" | head -1)
[ -n "$SYM" ] || { echo "no kernel matches $PAT"; exit 1; }
echo "$SYM"
$B/llvm-objdump -d --disassemble-symbols=$SYM $TMP/dev.co | awk '$1 ~ /^[sv]_|^ds_|^global_|^buffer_|^flat_|^scratch_/ {print $1}' > $TMP/ops
if [ -n "$OP" ]; then
    N=$(grep -cE "$OP" $TMP/ops)
    [ "$N" = 0 ] && echo "      0 $OP" || grep -E "$OP" $TMP/ops | sort | uniq -c | sort -rn
else
    sort $TMP/ops | uniq -c | sort -rn
fi
rm -rf $TMP
