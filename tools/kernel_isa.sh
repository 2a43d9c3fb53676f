#!/bin/bash
# The gfx950 assembly of one kernel, from hipcc -S on the device half (no GPU needed):
#   bash tools/kernel_isa.sh 'k_panel_ham_scan<qe::SearchEq3>' > /tmp/k.s
# The argument is matched against the demangled names; the first kernel whose name contains it is printed, from its label to
# its .amdhsa_kernel block.  Inner loops carry the compiler's "Inner Loop Header" comments.  A compile that fails, or a name
# that matches no kernel, ends the script with a message and a non-zero status.
set -euo pipefail
[ $# -eq 1 ] || { echo "usage: $0 NAME" >&2; exit 2; }
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
printf '#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "qe_types.h"\n#include "qe_kernels.hip"\n' > "$tmp/t.hip"
if ! /opt/rocm/bin/hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -S -I"$root/include" -I"$root/quicked_amd/csrc" \
     "$tmp/t.hip" -o "$tmp/t.s" 2> "$tmp/err"; then
    echo "$0: the compile failed:" >&2
    cat "$tmp/err" >&2
    exit 1
fi
sym=""
while read -r s; do
    if c++filt "$s" | grep -qF -- "$1"; then sym=$s; break; fi
done < <(grep -oE '^_Z[A-Za-z0-9_]+:' "$tmp/t.s" | tr -d ':')
[ -n "$sym" ] || { echo "$0: no kernel's name contains '$1'" >&2; exit 1; }
awk -v s="$sym" '$0 ~ "^"s":" { on = 1 } on { print } on && $0 ~ "\\.amdhsa_kernel "s { exit }' "$tmp/t.s"
