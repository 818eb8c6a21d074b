#!/bin/bash
# Register / LDS / scratch figures of every kernel in the shipped sources, one line per kernel:
#   tools/kernel_resources.sh > profiles/<round>_kernel_resources.txt
# (hipcc's -Rpass-analysis=kernel-resource-usage remarks on csrc/Makefile's `asm` target: its sources, its flags
#  per file; no GPU needed)
set -e
CSRC="$(cd "$(dirname "$0")/../imagematching_oetr_amd/csrc" && pwd)"
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
echo "# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage of the shipped sources ($(git -C "$CSRC" log -1 --format=%h 2>/dev/null || echo tree)), one line per kernel"
echo "# VGPRs | AGPRs | scratch B/lane | VGPR spills | SGPR spills | LDS B/block | waves/SIMD | kernel"
make -s -C "$TMP" -f "$CSRC/Makefile" VPATH="$CSRC" RESOURCES=1 asm 2>&1 |
    python3 -c '
import re, sys
cur = {}
for line in sys.stdin:
    m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
    if not m: continue
    k, v = m.groups()
    if k == "Function Name":
        cur = {"name": v}
    else:
        cur[k] = v
    if k == "LDS Size [bytes/block]":
        print("%4s | %3s | %4s | %3s | %3s | %7s | %2s | %s" % (cur.get("VGPRs"), cur.get("AGPRs"), cur.get("ScratchSize [bytes/lane]"), cur.get("VGPRs Spill"), cur.get("SGPRs Spill"), cur.get("LDS Size [bytes/block]"), cur.get("Occupancy [waves/SIMD]"), cur["name"]))
'
