#!/bin/bash
# Compares the gfx950 machine code of ptk_kernels.hip's kernels in the working tree with a commit's, kernel by kernel:
#   tools/kernel_isa_diff.sh [commit (default HEAD)] [kernel-name regex (default: the trace kernels and accumulate_kernel)]
# Builds the device code of all three builds (exact, PTK_CONTRACT=1, PTK_CONTRACT=2) of both trees, disassembles it without
# addresses or encodings (branch offsets are relative, so a kernel that only moved compares equal), and diffs each kernel
# matching the regex.  Exit status 0: every such kernel is identical.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
PAT=${2:-'trace_kernel|accumulate_kernel'}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
LLVM=${LLVM:-/opt/rocm/llvm/bin}
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/old"
git -C "$ROOT" archive "$REV" pbrpathtracer_amd/csrc include | tar -x -C "$TMP/old"

disasm() {  # <tree> <outdir>
    local csrc=$1/pbrpathtracer_amd/csrc out=$2
    mkdir -p "$out"
    for lvl in 0 1 2; do
        local extra=""
        [ "$lvl" != 0 ] && extra="-DPTK_CONTRACT=$lvl -ffp-contract=fast"
        (cd "$csrc" && $HIPCC -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -Wall -Wno-unused-function -fno-slp-vectorize \
            --offload-arch=gfx950 $extra --offload-device-only -c ptk_kernels.hip -o "$out/k$lvl.bundle")
        $LLVM/clang-offload-bundler --unbundle --type=o --input="$out/k$lvl.bundle" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$out/k$lvl.co"
        $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$out/k$lvl.co" | sed -e 's@//.*$@@' -e 's/[ \t]*$//' |
            awk -v dir="$out" -v lvl="$lvl" '/^<.*>:$/ { f = dir "/" lvl "." substr($0, 2, length($0) - 3) ".s"; next } f { print > f }'
    done
}
disasm "$TMP/old" "$TMP/a"
disasm "$ROOT" "$TMP/b"
status=0; n=0
for f in $(cd "$TMP/a" && ls *.s | grep -E "$PAT"); do
    n=$((n + 1))
    g=$f
    # a kernel template that gained a trailing bool parameter since: the old instantiation is the new one with it false
    [ -f "$TMP/b/$g" ] || g=$(echo "$f" | sed 's/EEEv/ELb0EEEv/')
    if [ ! -f "$TMP/b/$g" ]; then echo "missing in the working tree: $f"; status=1
    elif ! diff -q "$TMP/a/$f" "$TMP/b/$g" > /dev/null; then echo "DIFFERS: $f"; diff "$TMP/a/$f" "$TMP/b/$g" | head -20; status=1
    else echo "identical: $f ($(wc -l < "$TMP/a/$f") lines)$([ "$g" = "$f" ] || echo " = $g")"; fi
done
[ "$n" -gt 0 ] || { echo "no kernel matches $PAT"; exit 2; }
exit $status
