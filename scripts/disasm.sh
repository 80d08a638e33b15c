#!/bin/bash
# gfx950 disassembly of a built HIP object (no GPU needed): scripts/disasm.sh [obj] > out.s
# (no part0 is built any more: the filter below only keeps a stale one of an old build/obj out, which
# holds no device code to dump)
set -e
B=/opt/rocm/lib/llvm/bin
objs=${@:-$(ls build/obj/hip_step.hip.part*.o | grep -v part0)}
tmp=$(mktemp -d)
for obj in $objs; do
  $B/llvm-objcopy --dump-section=.hip_fatbin=$tmp/fatbin "$obj"
  $B/clang-offload-bundler --unbundle --type=o --input=$tmp/fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/co
  $B/llvm-objdump -d --mcpu=gfx950 $tmp/co
done
rm -rf $tmp
