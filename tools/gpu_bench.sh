#!/bin/bash
# the whole bench line alone (every leg: --full): $OUT/bench_<TAG>.json, OUT defaults to bench_out
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-r4}
timeout -k 10 ${TMO:-500} python -u bench.py --full ${BENCH_ARGS} > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err || { echo "BENCH FAILED"; tail $OUT/bench_${TAG}.err; exit 1; }
python3 tools/show_bench.py $OUT/bench_${TAG}.json 2>/dev/null || cut -c1-600 $OUT/bench_${TAG}.json
