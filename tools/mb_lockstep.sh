#!/bin/bash
# The two workgroups of a CU in the headline kernel, before (-DCP_BALANCE_PCT=0) and after (the library's setting) the priority trade
# of cp_fftlog_kernel.h (balances_cu): times, the per-CU offsets and rates of the CP_STAMPS build (tools/fftlog_microbench.hip), and one
# counter pass each, on its own.  On the GPU box: bash tools/mb_lockstep.sh [output directory]
set -o pipefail
O=${1:-/tmp/mb/lockstep}
mkdir -p /tmp/mb $O
build() { hipcc --offload-arch=gfx950 -O3 -std=c++17 "$@" tools/fftlog_microbench.hip 2>&1 | grep -E "error"; }
build -DCP_BALANCE_PCT=0 -o /tmp/mb/before &
build -o /tmp/mb/after &
build -DCP_STAMPS -DCP_BALANCE_PCT=0 -o /tmp/mb/stamps_before &
build -DCP_STAMPS -o /tmp/mb/stamps_after &
wait
run() { echo "== $1"; timeout -k 10 60 /tmp/mb/$1 100000 50; }
CNT="SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES"
{ run before && run after && run before && run after && run before && run after && run stamps_before && run stamps_after; } > $O/mb.txt 2>&1 &&
  timeout -k 10 300 rocprofv3 --pmc $CNT --output-format csv -d $O/pmc_before -- /tmp/mb/before 100000 5 0 > $O/pmc_before.log 2>&1 &&
  timeout -k 10 300 rocprofv3 --pmc $CNT --output-format csv -d $O/pmc_after -- /tmp/mb/after 100000 5 0 > $O/pmc_after.log 2>&1 || exit $?
cat $O/mb.txt
python3 tools/pmc_means.py $O/pmc_before $O/pmc_after
