#!/bin/bash
# Register / scratch / spill summary per kernel of one translation unit (compile only, no GPU):
#   tools/kres.sh discrete_mean_field_game_amd/csrc/mfg_core_small.hip [extra hipcc flags]
# Uses the flags of csrc/Makefile for that unit (make flags U=<unit>).
src=$1; shift
C=$(cd "$(dirname "$0")/../discrete_mean_field_game_amd/csrc" && pwd)
u=$(basename "$src" .hip)
/opt/rocm/bin/hipcc $(make -s -C $C flags U=$u) "$@" \
  -Rpass-analysis=kernel-resource-usage -c -o /dev/null "$src" 2>&1 | sed 's/ *\[-Rpass-analysis=kernel-resource-usage\]//' | awk '
  /Function Name:/ {name=$5}
  /VGPRs:/ && !/Spill/ {v=$NF}
  /ScratchSize/ {sc=$(NF)}
  /Occupancy/ {oc=$NF}
  /SGPRs Spill/ {ss=$NF}
  /VGPRs Spill/ {vs=$NF; printf "%-70s vgpr %3s occ %s scratch %4s sgpr_spill %3s vgpr_spill %3s\n", name, v, oc, sc, ss, vs}'
