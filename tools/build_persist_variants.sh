#!/bin/bash
# Variants of the persistent solver's float64 build only (bsgp_persist.hip),
# linked with the prebuilt objects of every other translation unit (build/*.o
# from __graft_entry__.build()):
#   tools/build_persist_variants.sh NAME "-DFLAG=V ..." [NAME "FLAGS" ...]
# -> beta-sgp_amd/libbsgp_NAME.so (for scripts/gpu_ab.sh)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
B=$R/build
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mcode-object-version=5"
# every other .hip of csrc/ is a translation unit of the library
OTHERS=""
for src in $R/beta-sgp_amd/csrc/*.hip; do
  f=$(basename $src .hip)
  [ $f = bsgp_persist ] || OTHERS="$OTHERS $B/$f.o"
done
while [ $# -ge 2 ]; do
  ( /opt/rocm/bin/hipcc $FLAGS $2 -I $R/include -c $R/beta-sgp_amd/csrc/bsgp_persist.hip -o $B/persist_$1.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/beta-sgp_amd/libbsgp_$1.so $B/persist_$1.o $OTHERS ) &
  shift 2
done
wait
