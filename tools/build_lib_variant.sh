#!/bin/bash
# Whole-library variant for A/B runs (scripts/gpu_ab.sh):
#   tools/build_lib_variant.sh NAME "-DFLAG=V ..." [SOURCE_ROOT]
# compiles every translation unit of SOURCE_ROOT (default: this tree; e.g. a
# `git worktree` of an older commit) in parallel -> beta-sgp_amd/libbsgp_NAME.so
# Every .hip file of SOURCE_ROOT's beta-sgp_amd/csrc/ is a translation unit of
# the library (DESIGN, host layer): the list is that directory's, so an older
# commit with other file names builds too.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2; SRC=${3:-$R}
B=/tmp/bsgp_build_$NAME; mkdir -p $B
CF="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mcode-object-version=5"
OBJS=(); PIDS=()
rm -f $B/*.o
for src in $SRC/beta-sgp_amd/csrc/*.hip; do
  f=$(basename $src .hip)
  /opt/rocm/bin/hipcc $CF $FLAGS -I $SRC/include -c $src -o $B/$f.o &
  PIDS+=($!); OBJS+=($B/$f.o)
done
for p in "${PIDS[@]}"; do wait $p || { echo "variant $NAME: a translation unit failed"; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/beta-sgp_amd/libbsgp_$NAME.so "${OBJS[@]}"
