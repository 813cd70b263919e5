#!/bin/bash
# Round-end measurement on the GPU box.  For each config in CONFIGS (default: headline): PMC
# passes -> profiles/pmc_traffic.json[configs][cfg] (read by bench.py --full for that config's
# roofline.traffic / valu_busy), kernel-trace stats, and that config's full bench line.
# Everything lands in $OUT_DIR (default bench_out/; copied into profiles/ afterwards).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
export OUT_DIR=${OUT_DIR:-bench_out}
O=$OUT_DIR
mkdir -p $O
for cfg in ${CONFIGS:-headline}; do
  CONFIG=$cfg bash tools/pmc_bench.sh || exit $?
  python3 tools/pmc_summary.py $O $O/pmc_summary_$cfg.csv \
    profiles/pmc_traffic.json $cfg || exit $?
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_stats_$cfg -o run \
    -- python3 bench.py --full --config $cfg --steps 20 --warmup 5 --no-cpu-baseline --no-lane-occupancy --train-steps 5 \
    > $O/prof_bench_$cfg.log 2>&1 || exit $?
  python3 tools/rocpd_stats.py $O/prof_stats_$cfg/run_results.db \
    $O/kernel_stats_$cfg.csv || exit $?
  # only the summaries are kept (the raw profiles run to hundreds of MiB)
  rm -rf $O/pmc $O/prof_stats_$cfg
  timeout -k 10 600 python3 bench.py --full --config $cfg > $O/bench_$cfg.log 2>&1 || exit $?
  tail -n 1 $O/bench_$cfg.log
done
cp profiles/pmc_traffic.json $O/pmc_traffic.json
