#!/bin/bash
# device_code_diff.sh A/libpstat.so B/libpstat.so -- are the gfx950 code objects of two builds the same device code?
#
# The argument that a host-only change cannot move a kernel's speed.  Each library's .hip_fatbin section is a run of clang
# offload bundles, one per object file; every gfx950 code object is taken out (clang-offload-bundler --unbundle) and
# disassembled (llvm-objdump: .text, and .rodata, where the kernel descriptors `<kernel>.kd` print as their .amdhsa_
# directives).  The listing is cut into one block per symbol, instruction addresses are dropped (encodings and
# symbol-relative branch targets stay), and the blocks are sorted by symbol name, because the order of instantiation inside
# an object may move.  Equal means: the same set of symbols, the same instruction text for each, the same descriptor for
# each kernel.  Prints a summary and exits 0 when equal; otherwise prints the name of every symbol that differs
# or that only one build has (a kernel whose parameter types changed has another mangled name), the diff's head, and exits 1.
set -euo pipefail
[ $# -eq 2 ] || { echo "usage: $0 A/libpstat.so B/libpstat.so" >&2; exit 2; }
LLVM=${LLVM:-/opt/rocm/llvm/bin}
ARCH=${ARCH:-gfx950}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT

listing() {   # $1 library, $2 work directory -> $2/listing: "symbol <tab> line", sorted by symbol
  mkdir -p "$2"
  "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$2/fatbin"
  local size offs i=0
  size=$(stat -c %s "$2/fatbin")
  offs=($(grep -a -o -b __CLANG_OFFLOAD_BUNDLE__ "$2/fatbin" | cut -d: -f1) "$size")
  : > "$2/raw"
  while [ $((i + 1)) -lt ${#offs[@]} ]; do
    head -c "${offs[i + 1]}" "$2/fatbin" | tail -c +$((offs[i] + 1)) > "$2/bundle"
    "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH \
        --input="$2/bundle" --output="$2/co"
    if [ -s "$2/co" ]; then
      { "$LLVM/llvm-objdump" -d "$2/co"; "$LLVM/llvm-objdump" -D -j .rodata "$2/co"; } |
        sed -E 's#// [0-9A-F]+: #// #' |
        awk '/file format|^Disassembly of section/ { sym = ""; next }
             /^[0-9a-f]+ <.*>:$/ { sym = $2; sub(/^</, "", sym); sub(/>:$/, "", sym); next }
             sym != "" && NF { print sym "\t" $0 }' >> "$2/raw"
    fi
    i=$((i + 1))
  done
  LC_ALL=C sort -s -t "$(printf '\t')" -k1,1 "$2/raw" > "$2/listing"
  echo "$1: $i bundles, $(cut -f1 "$2/listing" | uniq | grep -c '\.kd$') kernels," \
       "$(cut -f1 "$2/listing" | uniq | wc -l) symbols, $(wc -l < "$2/listing") lines of disassembly"
}

listing "$1" "$TMP/a"
listing "$2" "$TMP/b"
if ! diff <(cut -f1 "$TMP/a/listing" | uniq) <(cut -f1 "$TMP/b/listing" | uniq) > "$TMP/symdiff"; then
  echo "DIFFERENT: the sets of symbols differ"; head -20 "$TMP/symdiff"
fi
if ! diff "$TMP/a/listing" "$TMP/b/listing" > "$TMP/diff"; then
  cut -f1 "$TMP/diff" | grep '^[<>]' | sed 's/^[<>] //' | LC_ALL=C sort -u > "$TMP/names"
  echo "DIFFERENT: $(wc -l < "$TMP/names") symbols differ"
  cat "$TMP/names"
  head -40 "$TMP/diff"; exit 1
fi
echo "IDENTICAL: same symbols, same instructions per symbol, same kernel descriptors (compared per symbol, sorted by name)"
