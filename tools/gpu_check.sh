#!/bin/bash
# GPU-box round check: parity tests, headline bench (with CPU baseline), rocprofv3 kernel-trace summary.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT=${BENCH_OUT:-bench_out}  # where this script writes its logs and bench lines
export TMPDIR=/tmp
mkdir -p "$OUT"
TAG=${1:-cur}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests_$TAG.log 2>&1; rc=$?
tail -3 $OUT/gpu_tests_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
cat $OUT/bench_$TAG.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --events > $OUT/bench_prof_$TAG.json 2> $OUT/prof_$TAG.err || exit $?
python tools/stamp_stats.py $OUT/bench_prof_$TAG.json $OUT/prof_$TAG/run_kernel_stats.csv cornell_box_path || exit 1
cat $OUT/prof_$TAG/run_kernel_stats.csv
