#!/bin/bash
# Timing ablations of the small-d fused kernel (developer tool; results are WRONG by construction, only the time counts).
# Build (no GPU needed):   bash tools/ablate.sh build
# Run on the GPU box:      bash tools/ablate.sh run [d,B,T]
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/discrete_mean_field_game_amd/csrc; V=${MFG_VARIANT_DIR:-$C/variants}
ABL="PHILOX BM SETUP TRY HTAB LNY EPI COLREW V COLT TSUM"
if [ "$1" = build ]; then
  for a in $ABL; do
    # the three mixed-precision sampling units carry the switch.  Where the iterative-ILP scheduler fails on an ablated body,
    # the second call builds what is still missing without it (ILP= empties that flag group of csrc/Makefile).
    M="make -C $C -j${MFG_JOBS:-16} O=$V/abl_$a.obj OUT=$V/libabl_$a.so EXTRA_mfg_core_small=-DMFG_ABL_$a EXTRA_mfg_core_large_mixed=-DMFG_ABL_$a EXTRA_mfg_core_large_mixed_ilp=-DMFG_ABL_$a"
    $M >/dev/null 2>&1 || $M ILP= >/dev/null
  done
  ls $V
else
  S=${2:-21,65536,15}
  echo "baseline"; python3 $R/tools/core_probe.py $S 2>/dev/null | grep -E "rollout"
  for a in $ABL; do echo "without $a"; MFG_HIP_LIB=$V/libabl_$a.so python3 $R/tools/core_probe.py $S 2>/dev/null | grep -E "rollout"; done
fi
