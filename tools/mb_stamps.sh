#!/bin/bash
# fine-grained stamps (CP_STAMPS): where each phase of the flagship kernel spends its time, over all waves and by wave index within the workgroup
#   bash tools/mb_stamps.sh [extra flags for every build, e.g. "-DCP_WAVE_SKEW=5 -DCP_WAVE_ORDER=0x3120"]
# (profiles/headline_wave_skew_before.txt / _after.txt: without flags / with the skew on)
mkdir -p /tmp/mb
build() { hipcc --offload-arch=gfx950 -O3 -std=c++17 "$@" tools/fftlog_microbench.hip 2>&1 | grep -E "error" ; }
build -DCP_STAMPS $1 -o /tmp/mb/s0 &
build -DCP_STAMPS -DMB_WGS_PER_CU=1 $1 -o /tmp/mb/s0w1 &
build $1 -o /tmp/mb/m0 &
wait
for x in m0 s0 s0w1; do echo "== $x"; timeout -k 10 90 /tmp/mb/$x 100000 5 || exit $?; done
