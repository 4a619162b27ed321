#!/bin/bash
# One GPU-box round: parity tests -> smoke -> bench -> rocprofv3 kernel trace.  Logs under $OUT/.
set -o pipefail
OUT=${OUT:-out}  # logs and result lines
mkdir -p $OUT
export TMPDIR=/tmp
echo "== pytest -m gpu" | tee $OUT/progress.log
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; rc=$?
tail -15 $OUT/pytest_gpu.log
echo "pytest rc=$rc" | tee -a $OUT/progress.log
[ $rc -ne 0 ] && exit $rc
echo "== smoke" | tee -a $OUT/progress.log
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
tail -2 $OUT/smoke.log
for wl in ${WORKLOADS:-cat_1080p dog_1080p dog_4k}; do
  echo "== bench $wl" | tee -a $OUT/progress.log
  timeout -k 10 400 python bench.py --full --workload $wl > $OUT/bench_$wl.json 2> $OUT/bench_$wl.err || { tail -20 $OUT/bench_$wl.err; exit 1; }
  cat $OUT/bench_$wl.json
done
echo "== rocprofv3" | tee -a $OUT/progress.log
rm -rf $OUT/prof
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python bench.py --steps 20 --warmup 3 > $OUT/prof_bench.json 2> $OUT/prof.err || { tail -20 $OUT/prof.err; exit 1; }
find $OUT/prof -name "*stats*" | head
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
echo "== done" | tee -a $OUT/progress.log
