#!/bin/bash
# Everything the round's profiles/ needs, in one command on the GPU box: full GPU tests, rocprofv3 stats + PMC traffic of the default
# bench command, the bench lines (--full) of every configuration.  Results land in $OUT (default collect_out/); copy them into profiles/
# afterwards.
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
export OUT=${OUT:-$R/collect_out}
mkdir -p $OUT
# the driver's own command first (-x), then nothing is hidden: the full -rA report is kept
timeout -s KILL 1500 python -m pytest tests -x -q -m gpu -rA 2>&1 | tail -420 > $OUT/pytest_gpu_full.log
grep -E "passed|failed" $OUT/pytest_gpu_full.log | tail -2 | tee $OUT/pytest_gpu.log
grep -E "^FAILED|^ERROR" $OUT/pytest_gpu_full.log | head
bash tools/collect_profiles.sh
cd $R
# SQ counters (wave-cycle split, MFMA busy cycles, LDS activity) of the default kernels
bash tools/collect_sq_pmc.sh > /dev/null 2>&1; cp $OUT/pmc_sq_summary.txt $OUT/pmc_sq_summary_default.txt
cd $R
timeout -s KILL 400 python bench.py --full > $OUT/line_default.log 2>&1
timeout -s KILL 200 python bench.py --full --optimizer adam --no-cpu-baseline > $OUT/line_adam.log 2>&1
timeout -s KILL 200 python bench.py --full --ids zipf --no-cpu-baseline > $OUT/line_zipf.log 2>&1
timeout -s KILL 200 python bench.py --full --preset c2 --no-cpu-baseline > $OUT/line_c2.log 2>&1
timeout -s KILL 400 python bench.py --full --model dcn > $OUT/line_dcn.log 2>&1
timeout -s KILL 400 python bench.py --full --model dssm > $OUT/line_dssm.log 2>&1
DR_FUSE_K3=0 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_unfused.log 2>&1
DR_NO_CONCAT=0 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_concat.log 2>&1
DR_FORCE_SHARDED=1 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_sharded_world1.log 2>&1
DR_FORCE_SHARDED=1 timeout -s KILL 300 python bench.py --full --model dcn --no-cpu-baseline > $OUT/line_dcn_sharded_world1.log 2>&1
DR_PREFETCH_EARLY=0 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_plan_beside_k4.log 2>&1
# one step as a timeline
bash tools/exp/timeline_call.sh default bf3_emb_linear_kernel -- > /dev/null 2>&1
bash tools/exp/timeline_call.sh sharded bf3_gemm_tn_rs_kernel DR_FORCE_SHARDED=1 -- > /dev/null 2>&1
cd $R
# round 6: the three-kernel backward of round 5 (dgrad, wgrad, K4) beside the fused default
DR_FUSE_K4=0 DR_BENCH_STRICT=0 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_k4_unfused.log 2>&1
# round 6 experiment drivers: the 16-wave kernel against the 8-wave one (bit-identity + times; the 8-wave leg needs a library built with
# DR_HIPCC_EXTRA=-DDR_OCC_ABLATE, see occ_bench.py), the fused dgrad + K4 against dgrad + K4
timeout -s KILL 300 python tools/exp/occ_bench.py 2>&1 | grep "OCC=" > $OUT/occ_bench.log
timeout -s KILL 300 python tools/exp/fused_k4_bench.py 2>&1 | grep FUSEDK4 > $OUT/fused_k4_bench.log
timeout -s KILL 300 python tools/exp/fused_k4_bench.py 2000000 zipf 2>&1 | grep FUSEDK4 >> $OUT/fused_k4_bench.log
# the six-product mode of rounds 2-3 beside the default (f16x2) lines: default, DCN, sharded
DR_GEMM_SPLIT=bf16x3 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_bf16x3.log 2>&1
DR_GEMM_SPLIT=bf16x3 timeout -s KILL 300 python bench.py --full --model dcn --no-cpu-baseline > $OUT/line_dcn_bf16x3.log 2>&1
DR_GEMM_SPLIT=bf16x3 DR_FORCE_SHARDED=1 timeout -s KILL 200 python bench.py --full --no-cpu-baseline > $OUT/line_sharded_world1_bf16x3.log 2>&1
timeout -s KILL 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
for f in default adam zipf c2 dcn dssm unfused concat sharded_world1 dcn_sharded_world1 plan_beside_k4 k4_unfused bf16x3 dcn_bf16x3 sharded_world1_bf16x3; do
  python - $f <<'PY'
import json, os, sys
try:
    d = json.loads(open(os.path.join(os.environ["OUT"], "line_%s.log" % sys.argv[1])).read().strip().splitlines()[-1])
    r = d.get("roofline") or {}
    print(sys.argv[1], d["value"], d["ms_per_step"], r.get("kernel"), r.get("frac"), (d.get("cpu_baseline") or {}).get("value"))
except Exception as e:
    print(sys.argv[1], "FAILED", e)
PY
done
# the raw per-dispatch traces are tens of MB: the summaries above are what profiles/ keeps
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE $OUT/pmc_sq $OUT/prof_stats $OUT/tl_default $OUT/tl_sharded
du -sh $OUT
