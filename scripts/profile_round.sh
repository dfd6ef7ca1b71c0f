#!/bin/bash
# rocprofv3 evidence for one round (run on the GPU box through gpurun):  bash scripts/profile_round.sh [c2] [c4]
# Kernel-trace/stats passes and PMC passes are separate runs (gpurun refuses mixed ones); FETCH_SIZE and WRITE_SIZE need
# separate passes (TCC slot limit).  Output: gpurun_out/profiles/{summary.json, c2_counters.json, c4_counters.json,
# *_kernel_stats.csv}; copy what should be judged into profiles/rNN/.
set -o pipefail
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
export TMPDIR=/tmp
# the profiler's preloaded library starts the HIP runtime before python runs bench.py's os.environ.setdefault: export the
# queue count here so that the profiled overlap is the benched one
export GPU_MAX_HW_QUEUES=16
OUT=$PWD/gpurun_out/profiles; mkdir -p "$OUT"
WHAT="${*:-c2 c4}"
# the benched commands, each with its steps + warm-up steps beside it (what a pass's time limit is made of)
C2="python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-secondary"; N_C2=12
C4="python3 bench.py --full --config c4 --steps 5 --warmup 1 --no-cpu-baseline"; N_C4=6
C3="python3 bench.py --full --config c3 --steps 3 --warmup 1 --no-cpu-baseline"; N_C3=4
C5="python3 bench.py --full --config c5 --steps 5 --warmup 1 --no-cpu-baseline"; N_C5=6
C4XL="python3 bench.py --full --config c4xl --steps 3 --warmup 1 --no-cpu-baseline"; N_C4XL=4
# one profiler pass under a time limit of its own, LIMIT = 40 s (profiler, runtime, the scene's build) + 3 s per step of the benched command:
# 76 s on C2 (a pass was measured at 1.8 s), 58 s on C4 and C5 (2 - 2.6 s), 52 s on C3 (2.5 s) and on c4xl (8 s, most of it the build of its ten
# million triangles) -- six times the slowest pass, more on the others.  A pass that fails or runs out of time ENDS the script: nothing more is
# started on a card that may have faulted
run() {
  name=$1; shift; rm -rf "$OUT/$name"
  timeout -k 10 $LIMIT rocprofv3 "$@" > "$OUT/$name.log" 2>&1 || { echo "FAILED $name (exit $?, limit $LIMIT s)"; tail -5 "$OUT/$name.log"; exit 1; }
}
for cfg in $WHAT; do
  if [ "$cfg" = c2 ]; then CMD=$C2; N=$N_C2; elif [ "$cfg" = c3 ]; then CMD=$C3; N=$N_C3; elif [ "$cfg" = c5 ]; then CMD=$C5; N=$N_C5; elif [ "$cfg" = c4xl ]; then CMD=$C4XL; N=$N_C4XL; else CMD=$C4; N=$N_C4; fi
  LIMIT=$((40 + 3 * N))
  run ${cfg}_trace --kernel-trace --stats --output-format csv -d "$OUT/${cfg}_trace" -- $CMD
  run ${cfg}_fetch --pmc FETCH_SIZE --output-format csv -d "$OUT/${cfg}_fetch" -- $CMD
  run ${cfg}_write --pmc WRITE_SIZE --output-format csv -d "$OUT/${cfg}_write" -- $CMD
  run ${cfg}_sq1 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY --output-format csv -d "$OUT/${cfg}_sq1" -- $CMD
  run ${cfg}_sq2 --pmc SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE --output-format csv -d "$OUT/${cfg}_sq2" -- $CMD
  run ${cfg}_dram --pmc TCC_EA0_RDREQ_DRAM_32B_sum TCC_EA0_RDREQ_sum --output-format csv -d "$OUT/${cfg}_dram" -- $CMD
  if [ "$cfg" = c4 ] || [ "$cfg" = c4xl ]; then
    run ${cfg}_tcc --pmc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum --output-format csv -d "$OUT/${cfg}_tcc" -- $CMD
  fi
  if [ "$cfg" = c4 ]; then
    run c4_ta --pmc TA_BUSY_avr TA_TA_BUSY_sum GRBM_GUI_ACTIVE SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_FLAT --output-format csv -d "$OUT/c4_ta" -- $CMD
  fi
done
python3 scripts/pmc_summary.py "$OUT" $WHAT
