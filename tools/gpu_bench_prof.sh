#!/bin/bash
# the whole bench line (every leg: --full) + rocprofv3 kernel stats and fabric counters
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${TAG:-r4}
timeout -k 10 500 python -u bench.py --full > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err || { echo "BENCH FAILED"; tail $OUT/bench_${TAG}.err; exit 1; }
cat $OUT/bench_${TAG}.json | cut -c1-600
bash tools/profile_round.sh $TAG || { echo "PROFILE FAILED"; exit 1; }
echo ok
