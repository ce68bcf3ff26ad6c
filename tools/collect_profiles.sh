#!/bin/bash
# Collect the round's judged profiles on the GPU box (run through gpurun):
#   $OUT/prof_stats/   rocprofv3 --kernel-trace --stats of the default bench command (--full: the kernels timed alone are in it)
#   $OUT/pmc_traffic.json   per-kernel HBM bytes (FETCH_SIZE / WRITE_SIZE in separate --pmc passes)
# Copy the results into profiles/ afterwards (tools/rocpd_stats.py turns the kernel trace into a CSV summary).
# CAUTION (round 4, 37 GPU-minutes lost): always `--output-format csv` and `timeout -s KILL`.  A rocprofv3 run WITHOUT the csv format writes a
# rocpd database and its --stats post-processing of a few thousand launches did not finish in 35 minutes; plain `timeout` signals
# rocprofv3 only, the profiled python keeps a pipe open and the call runs into gpurun's own limit.  Give the gpurun call a --timeout
# that matches the work (the budget left is the default ceiling).
set -u
export DR_BENCH_STRICT=0      # (the profiled passes time the shipped step only; the strict-fp32 sub-record is in the bench lines)
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd /tmp && export TMPDIR=/tmp
OUT=${OUT:-$R/collect_out}
mkdir -p $OUT
BENCH="python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline"
timeout -s KILL 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/prof_stats_bench.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 600 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- $BENCH > /dev/null 2>&1
done
python $R/tools/pmc_traffic.py $OUT/pmc_traffic.json $(find $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE -name "*counter_collection.csv") > $OUT/pmc_traffic.txt 2>&1
STATS=$(ls -t $(find $OUT/prof_stats -name "*kernel_stats.csv") | head -1)
[ -n "$STATS" ] && cp "$STATS" $OUT/kernel_stats.csv
TRACE=$(ls -t $(find $OUT/prof_stats -name "*kernel_trace.csv") | head -1)
[ -n "$TRACE" ] && python $R/tools/trace_timed_stats.py "$TRACE" --last 20 > $OUT/kernel_stats_timed.csv
tail -1 $OUT/prof_stats_bench.log | cut -c1-300
