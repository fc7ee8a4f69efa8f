#!/bin/bash
# Compares the gfx950 machine code of the library's kernels in the working tree with a commit's, kernel by kernel:
#   tools/kernel_isa_diff.sh [commit (default HEAD)] [kernel-name regex (default: the trace kernels and accumulate_kernel)] [extra sources]
# In each tree it builds the device code of ptk_kernels.hip at all three levels (exact, PTK_CONTRACT=1, PTK_CONTRACT=2) and, at
# the exact level, of ptk_frame.hip where the tree has it and of the extra sources named in the third argument or in EXTRA_SRCS
# (e.g. "ptk_adaptive.hip ptk_features.hip"); disassembles it without addresses or encodings (branch offsets are relative, so a
# kernel that only moved compares equal) into one file per level and kernel, whichever source it came from - a kernel that moved
# between files still compares by name - and diffs each kernel matching the regex.  Exit status 0: every such kernel is identical.
# A tree that has ptk_kernels_plain.hip (the exact PLAIN trace kernels' unit) gets that unit built at the exact level too, with the
# unit's own flags as csrc/Makefile states them (PLAIN_UNIT_FLAGS), so those two kernels compare as they are built; likewise
# ptk_kernels_rect.hip (the pair unit) with RECT_UNIT_FLAGS on top of those, and ptk_kernels_cycle.hip (the cycle unit) with CYCLE_UNIT_FLAGS.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
PAT=${2:-'trace_kernel|accumulate_kernel'}
EXTRA_SRCS=${3:-${EXTRA_SRCS:-}}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
LLVM=${LLVM:-/opt/rocm/llvm/bin}
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/old"
git -C "$ROOT" archive "$REV" pbrpathtracer_amd/csrc include | tar -x -C "$TMP/old"

one() {  # <csrc> <outdir> <level> <source>
    local csrc=$1 out=$2 lvl=$3 src=$4 extra="" obj
    obj="$out/$(basename "$src" .hip).$lvl"
    [ "$lvl" != 0 ] && extra="-DPTK_CONTRACT=$lvl -ffp-contract=fast"
    [ "$src" = ptk_kernels_plain.hip ] && extra=$(sed -n 's/^PLAIN_UNIT_FLAGS[ \t]*?=[ \t]*//p' "$csrc/Makefile")
    [ "$src" = ptk_kernels_rect.hip ] && extra="$(sed -n 's/^PLAIN_UNIT_FLAGS[ \t]*?=[ \t]*//p' "$csrc/Makefile") $(sed -n 's/^RECT_UNIT_FLAGS[ \t]*?=[ \t]*//p' "$csrc/Makefile")"
    [ "$src" = ptk_kernels_cycle.hip ] && extra="$(sed -n 's/^PLAIN_UNIT_FLAGS[ \t]*?=[ \t]*//p' "$csrc/Makefile") $(sed -n 's/^CYCLE_UNIT_FLAGS[ \t]*?=[ \t]*//p' "$csrc/Makefile")"
    (cd "$csrc" && $HIPCC -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -Wall -Wno-unused-function -fno-slp-vectorize \
        --offload-arch=gfx950 $extra --offload-device-only -c "$src" -o "$obj.bundle")
    $LLVM/clang-offload-bundler --unbundle --type=o --input="$obj.bundle" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$obj.co"
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$obj.co" | sed -e 's@//.*$@@' -e 's/[ \t]*$//' |
        awk -v dir="$out" -v lvl="$lvl" '/^<.*>:$/ { f = dir "/" lvl "." substr($0, 2, length($0) - 3) ".s"; next } f { print > f }'
}
disasm() {  # <tree> <outdir>
    local csrc=$1/pbrpathtracer_amd/csrc out=$2 src
    mkdir -p "$out"
    for lvl in 0 1 2; do one "$csrc" "$out" $lvl ptk_kernels.hip; done
    for src in ptk_frame.hip ptk_kernels_plain.hip ptk_kernels_rect.hip ptk_kernels_cycle.hip $EXTRA_SRCS; do
        [ -f "$csrc/$src" ] && one "$csrc" "$out" 0 "$src"
    done
    return 0
}
# without the padding behind a kernel's last instruction, which depends on what follows it in its code object
body() { awk '{ l[NR] = $0 } END { n = NR; while (n > 0 && l[n] ~ /^[ \t]*(s_nop 0|\.\.\.)?$/) n--; for (i = 1; i <= n; i++) print l[i] }' "$1"; }
disasm "$TMP/old" "$TMP/a"
disasm "$ROOT" "$TMP/b"
status=0; n=0
for f in $(cd "$TMP/a" && ls *.s | grep -E "$PAT"); do
    n=$((n + 1))
    g=$f
    # a kernel template that gained a trailing bool parameter since: the old instantiation is the new one with it false
    [ -f "$TMP/b/$g" ] || g=$(echo "$f" | sed 's/EEEv/ELb0EEEv/')
    if [ ! -f "$TMP/b/$g" ]; then echo "missing in the working tree: $f"; status=1
    elif ! diff -q <(body "$TMP/a/$f") <(body "$TMP/b/$g") > /dev/null; then echo "DIFFERS: $f"; { diff <(body "$TMP/a/$f") <(body "$TMP/b/$g") || true; } | head -20; status=1
    else echo "identical: $f ($(wc -l < "$TMP/a/$f") lines)$([ "$g" = "$f" ] || echo " = $g")"; fi
done
[ "$n" -gt 0 ] || { echo "no kernel matches $PAT"; exit 2; }
exit $status
