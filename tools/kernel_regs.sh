#!/bin/bash
# VGPRs / SGPRs / LDS and scratch bytes / spills / occupancy of the kernels of one .hip file whose mangled name matches a pattern.
#   tools/kernel_regs.sh [pattern] [file]       e.g. tools/kernel_regs.sh 'k_final_fast|k_down_march'
#                                               or   tools/kernel_regs.sh k_assess_march csrc/sr_assess.hip
#                                               or   tools/kernel_regs.sh 'k_feather_merge|k_seam_scan' csrc/sr_tiles.hip
cd "$(dirname "$0")/../super-resolution-system_amd" || exit 1
pat=${1:-.}
src=${2:-csrc/sr_engine.hip}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden -DSR_BUILD \
    -I ../include -I csrc $SR_HIPCC_EXTRA -x hip -c "$src" -o /tmp/kernel_regs.o -Rpass-analysis=kernel-resource-usage 2>&1 |
    awk '/Function Name:/ {name=$5} /TotalSGPRs:/ {sg=$4} /  VGPRs:/ {v=$4} /ScratchSize/ {sc=$5} /VGPRs Spill:/ {sp=$5} /SGPRs Spill:/ {ss=$5} /Occupancy/ {occ=$5} /LDS Size/ {printf "%-90s vgpr %3s  sgpr %3s  lds %6s  scratch %s  spill v%s s%s  waves %s\n", name, v, sg, $6, sc, sp, ss, occ}' |
    grep -E "$pat"
