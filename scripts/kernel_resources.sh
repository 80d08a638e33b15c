#!/bin/bash
# Register / scratch footprint of the step kernels in a built object (no GPU needed):
#   scripts/kernel_resources.sh [build/obj/hip_step.hip.part_g16.o]
# KERNEL=<pattern> lists the kernels whose name matches it instead, with their LDS bytes as well, e.g.
#   KERNEL=ray_query_kernel scripts/kernel_resources.sh build/obj/hip_render.hip.o
set -e
B=/opt/rocm/lib/llvm/bin
# (part0: a stale dispatcher object of an old build/obj; none is built any more)
objs=${@:-$(ls build/obj/hip_step.hip.part*.o | grep -v part0)}
fields='^\s+\.name:|\.vgpr_count|\.sgpr_count|\.private_segment_fixed_size|\.vgpr_spill_count|\.agpr_count'
[ -n "$KERNEL" ] && fields="$fields|\.group_segment_fixed_size"
tmp=$(mktemp -d)
for obj in $objs; do
  $B/llvm-objcopy --dump-section=.hip_fatbin=$tmp/fatbin "$obj"
  $B/clang-offload-bundler --unbundle --type=o --input=$tmp/fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/co
  $B/llvm-readelf --notes $tmp/co | grep -E "$fields" \
    | awk '/\.name:/{if(n)print n, r; n=$2; r=""; next} {r=r" "$1$2} END{print n, r}' | grep "${KERNEL:-step_kernel}" | c++filt || true
done
rm -rf $tmp
