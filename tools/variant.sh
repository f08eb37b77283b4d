#!/bin/bash
# Developer tool: build a variant of the library with extra -D flags on ONE translation unit (no GPU needed), for A/B
# timing through MFG_HIP_LIB:   bash tools/variant.sh <name> <file.hip> "<-D flags>"   ->  csrc/variants/lib<name>.so
# The units and their flags are csrc/Makefile's; the variant's objects go to csrc/variants/<name>.obj/.
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/discrete_mean_field_game_amd/csrc; V=${MFG_VARIANT_DIR:-$C/variants}   # (MFG_VARIANT_DIR=$C/ab: a directory that travels with gpurun)
NAME=$1; TU=$2; FLAGS=$3
make -C $C -j${MFG_JOBS:-16} O=$V/$NAME.obj OUT=$V/lib$NAME.so "EXTRA_${TU%.hip}=$FLAGS" >/dev/null && echo $V/lib$NAME.so
