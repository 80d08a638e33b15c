#!/bin/bash
# Is the gfx950 device code of two builds the same?  (no GPU needed)
#   scripts/same_code.sh PARENT_OBJDIR NEW_OBJDIR
# For every step part (hip_step.hip.part_*.o), hip_render.hip.o and hip_batch.hip.o of either directory: the
# disassembly (scripts/disasm.sh) compared function by function, keyed by symbol name, so the order in
# which the functions were emitted does not matter; the kernels' metadata (scripts/kernel_resources.sh:
# VGPRs, SGPRs, scratch, spills, LDS) and the bytes of .text.  One line per object; exit status 1 on any
# difference (the differing symbols listed), on an object that only one side has, and on an object in
# which no function or no kernel was found.
set -e
set -o pipefail
[ $# -eq 2 ] || { echo "usage: $0 PARENT_OBJDIR NEW_OBJDIR" >&2; exit 2; }
here=$(cd "$(dirname "$0")" && pwd)
B=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT

# "symbol <tab> instruction text and encoding" per instruction, without the addresses (a function that
# moved is still the same function), stably sorted by symbol: each function's lines stay in order
functions() {
  bash "$here/disasm.sh" "$1" | awk '
    /^[0-9a-f]+ <.*>:$/ { sym = $2; print sym "\t"; next }
    sym != "" && /\/\/ [0-9A-F]+:/ { sub(/\/\/ [0-9A-F]+:/, "//"); print sym "\t" $0 }' | LC_ALL=C sort -s -t "$(printf '\t')" -k1,1 > "$2"
}
text_bytes() {
  $B/llvm-objcopy --dump-section=.hip_fatbin=$tmp/fatbin "$1"
  $B/clang-offload-bundler --unbundle --type=o --input=$tmp/fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/co
  echo $((16#$($B/llvm-readelf -S -W $tmp/co | awk '/ \.text +PROGBITS/ { sub(/.*PROGBITS +[0-9a-f]+ +[0-9a-f]+ +/, ""); print $1 }')))
}

status=0
names=$(for d in "$1" "$2"; do (cd "$d" && ls hip_step.hip.part_*.o hip_render.hip.o hip_batch.hip.o 2>/dev/null) || true; done)
names=$(echo "$names" | sort -u)
[ -n "$names" ] || { echo "no objects in $1 or $2" >&2; exit 2; }
for name in $names; do
  old="$1/$name"
  new="$2/$name"
  [ -f "$old" ] || { echo "$name: ONLY in $2"; status=1; continue; }
  [ -f "$new" ] || { echo "$name: ONLY in $1"; status=1; continue; }
  functions "$old" $tmp/a
  functions "$new" $tmp/b
  nfun=$(cut -f1 $tmp/a | uniq | wc -l)
  KERNEL=. bash "$here/kernel_resources.sh" "$old" | sort > $tmp/ma
  KERNEL=. bash "$here/kernel_resources.sh" "$new" | sort > $tmp/mb
  nker=$(wc -l < $tmp/ma)
  ta=$(text_bytes "$old")
  tb=$(text_bytes "$new")
  if [ "$nfun" -eq 0 ] || [ "$nker" -eq 0 ]; then
    echo "$name: NOTHING FOUND ($nfun functions, $nker kernels)"
    status=1
  elif cmp -s $tmp/a $tmp/b && cmp -s $tmp/ma $tmp/mb && [ "$ta" = "$tb" ]; then
    echo "$name: same ($nfun functions, $nker kernels, .text $ta bytes)"
  else
    echo "$name: DIFFERENT (.text $ta -> $tb bytes)"
    { diff $tmp/a $tmp/b || true; } | awk -F '\t' '/^[<>]/ { sub(/^[<>] /, "", $1); print $1 }' | uniq | sort -u | head -20 | c++filt | sed 's/^/  /'
    { diff $tmp/ma $tmp/mb || true; } | head -20 | sed 's/^/  /'
    status=1
  fi
done
exit $status
