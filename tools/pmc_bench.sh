#!/bin/bash
# PMC passes over a short full bench run (one counter group per rocprofv3 run, kernel-trace
# only).  CONFIG=<bench config> (default headline).  Output: $OUT_DIR/pmc/<config>_<pass>/...
# counter_collection.csv per pass (OUT_DIR default bench_out).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
CONFIG=${CONFIG:-headline}
ARGS=${BENCH_ARGS:---full --steps 3 --warmup 1 --no-cpu-baseline --no-lane-occupancy --train-steps 1}
O=${OUT_DIR:-bench_out}/pmc
mkdir -p $O
run() {  # run <name> <counters...>
  local name=$1; shift
  timeout -k 10 300 rocprofv3 --pmc "$@" --output-format csv -d $O/${CONFIG}_$name \
    -o run -- python3 bench.py --config $CONFIG $ARGS > $O/${CONFIG}_$name.log 2>&1
}
run fetch FETCH_SIZE && run write WRITE_SIZE && \
run sq SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_INST_ANY \
  SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_TRANS_F32 && \
run sq2 SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SALU SQ_WAVES SQ_INSTS_VMEM_RD \
  SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS
