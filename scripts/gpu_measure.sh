#!/bin/bash
# Evidence for the bench line at HEAD (one call): bench --full (default config),
# rocprofv3 kernel stats of the default command and of --streams 1 (whose
# per-kernel averages are the launch unit of bench.py's profiled roofline),
# the PMC traffic passes and the SQ counter passes.  Usage: TAG [bench args]
# Output under $BENCH_OUT (default bench_out/).
set -o pipefail
TAG=${1:-meas}; shift
cd "$(dirname "$0")/.."; O=${BENCH_OUT:-bench_out}; mkdir -p $O
timeout -k 10 400 python -u bench.py --full --steps 5 --warmup 1 "$@" > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { echo "bench failed"; tail -5 $O/${TAG}_bench.err; exit 3; }
cat $O/${TAG}_bench.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/${TAG}_prof3 -o run --output-format csv -- python bench.py --steps 5 --warmup 1 "$@" > $O/${TAG}_prof3.log 2>&1 || { echo "prof3 failed"; exit 3; }
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/${TAG}_prof1 -o run --output-format csv -- python bench.py --streams 1 --steps 2 --warmup 1 "$@" > $O/${TAG}_prof1.log 2>&1 || { echo "prof1 failed"; exit 3; }
for d in prof3 prof1; do echo "== $d"; find $O/${TAG}_$d -name "*kernel_stats.csv" | head -1 | xargs -r cut -d, -f1-4 | grep -E "Name|bsgp::k_" ; done
bash scripts/gpu_traffic.sh ${TAG} "$@" || exit 3
bash scripts/gpu_sq.sh ${TAG}_sq "$@" || exit 3
