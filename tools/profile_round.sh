#!/bin/bash
# One GPU call that refreshes the round's measurement evidence (run from the repo root):
#   usage: tools/profile_round.sh [OUTDIR]     (default evidence_out; tools/roofline_evidence.py reads it)
#   1. bench.py --full default line (N=1, roofline, kernels, the CPU baseline) -> OUTDIR/bench.json
#   2. rocprofv3 --kernel-trace --stats of the same bench command        -> OUTDIR/prof_stats/
#   3. two PMC passes (FETCH_SIZE, WRITE_SIZE: they do not fit one pass) over the roofline kernel
#      set (tools/gemm_pmc.py layer)                                      -> OUTDIR/pmc_{fetch,write}/
# Every GPU step has its own time limit; the chain stops at the first failure.
set -o pipefail
R=$(pwd)
O=${1:-evidence_out}
mkdir -p "$O"
O=$(cd "$O" && pwd)
export TMPDIR=/tmp
timeout -k 10 420 python3 bench.py --full > "$O/bench.json" 2> "$O/bench.err" &&
cd /tmp &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/prof_stats" -o bench --output-format csv \
  -- python3 "$R/bench.py" --full --no-cpu-baseline > "$O/bench_prof.json" 2> "$O/prof_stats.err" &&
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d "$O/pmc_fetch" -o pmc --output-format csv \
  -- python3 "$R/tools/gemm_pmc.py" layer 20 > "$O/pmc_fetch.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d "$O/pmc_write" -o pmc --output-format csv \
  -- python3 "$R/tools/gemm_pmc.py" layer 20 > "$O/pmc_write.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_BUSY_CYCLES \
  -d "$O/pmc_mfma" -o pmc --output-format csv \
  -- python3 "$R/tools/gemm_pmc.py" layer 300 > "$O/pmc_mfma.log" 2>&1 &&
cd "$R" &&
timeout -k 10 200 python3 tools/gemm_clock.py 1.5 5 > "$O/clock.log" 2>&1
rc=$?
echo "profile_round rc=$rc"
exit $rc
