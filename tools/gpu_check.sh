#!/bin/bash
# GPU sanity pass: parity tests, smoke, the full bench record (bench.py --full), rocprof kernel stats of
# the plain run.  Everything goes under $OUT (default bench_out/).
set -o pipefail
out=${OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > $out/gpu_tests.log 2>&1 || { tail -30 $out/gpu_tests.log; exit 1; }
tail -3 $out/gpu_tests.log
timeout -k 10 200 python -u bench.py --full > $out/bench.json 2> $out/bench.err || { cat $out/bench.err | tail; exit 1; }
cat $out/bench.json
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $out/prof -o run -- python3 bench.py > $out/prof.log 2>&1 || { tail $out/prof.log; exit 1; }
find $out/prof -name '*kernel_stats.csv'
