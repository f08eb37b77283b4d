#!/bin/bash
# Developer tool: the -DMFG_TIMING build of the library (s_memtime stamps in the small-d fused kernel: tools/phase_timing.py,
# tools/phase_timing_t1.py).  CoreArgs gains a debug pointer, so EVERY translation unit is rebuilt with the flag.
#   bash tools/build_timing.sh   ->  csrc/variants/libtiming.so   (MFG_VARIANT_DIR=.../csrc/ab: a directory that travels with gpurun)
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/discrete_mean_field_game_amd/csrc; V=${MFG_VARIANT_DIR:-$C/variants}
make -C $C -j${MFG_JOBS:-16} O=$V/timing OUT=$V/libtiming.so EXTRA=-DMFG_TIMING >/dev/null && echo $V/libtiming.so
