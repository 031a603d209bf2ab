#!/bin/bash
# GPU-box helper: bench line (with CPU baseline) + rocprofv3 kernel-trace summary per config.
#   bash tools/gpu_configs.sh TAG CFG [CFG ...]
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT=${BENCH_OUT:-bench_out}  # where this script writes its logs and bench lines
export TMPDIR=/tmp
mkdir -p "$OUT"
TAG=$1; shift
for CFG in "$@"; do
  timeout -k 10 600 python bench.py --full --config "$CFG" --steps 3 --warmup 1 > $OUT/bench_${TAG}_$CFG.json 2> $OUT/bench_${TAG}_$CFG.err || exit $?
  cat $OUT/bench_${TAG}_$CFG.json
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_$CFG -o run -- \
      python bench.py --full --config "$CFG" --steps 3 --warmup 1 --no-cpu-baseline --events > $OUT/bench_prof_${TAG}_$CFG.json 2> $OUT/prof_${TAG}_$CFG.err || exit $?
  python tools/stamp_stats.py $OUT/bench_prof_${TAG}_$CFG.json $OUT/prof_${TAG}_$CFG/run_kernel_stats.csv $CFG || exit 1
  head -4 $OUT/prof_${TAG}_$CFG/run_kernel_stats.csv
done
