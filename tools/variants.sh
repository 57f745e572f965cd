#!/bin/bash
# Developer tool: build variants of libsmpc.so whose lane pass is compiled with extra flags, side by
# side under mpcholonavigation_amd/variants/, for tools/kbench_all.py to time against the product
# library in one call.   tools/variants.sh name "-DFLAG=0 ..." ...
# The rule: a compile-time switch for an experiment lives in a working tree while it is being
# measured.  What is committed is the winner, plus one sentence with the numbers where the loser
# would have stood (and in DESIGN.md); the committed sources define no such switch.
set -e
cd "$(dirname "$0")/../mpcholonavigation_amd/csrc"
make -s
mkdir -p ../variants
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function"
while [ $# -ge 2 ]; do
  name=$1; defs=$2; shift 2
  ( /opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -Wno-pass-failed $defs -c -o ../variants/lane_$name.o smpc_lane.hip
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../variants/libsmpc_$name.so smpc_kernels.o smpc_wave_many.o smpc_wave_stats.o smpc_wave_stats_many.o \
        ../variants/lane_$name.o smpc_split.o smpc_limit.o smpc_moving.o \
        smpc_api.o smpc_noise.o smpc_limit_host.o smpc_moving_host.o smpc_debug.o smpc_prepare.o smpc_shard.o smpc_group.o smpc_stats.o \
        -Wl,-rpath,/opt/rocm/lib
    echo built $name ) &
done
wait
