#!/bin/bash
# Developer tool: two builds of libsmpc.so against each other on the headline, in ONE call on one box.
#   tools/ab_libs.sh PARENT_DIR/libsmpc.so NEW_DIR/libsmpc.so OUTDIR [ROUNDS]
# Both files must be NAMED libsmpc.so: bench.py's timed ticks are issued by libsortham_host.so, which finds
# its libsmpc.so by name — in LD_LIBRARY_PATH, set here to the library's directory, before its own
# directory.  With SMPC_LIB alone the Python side runs the given library and the timed loop the tree's.
# Per round: parent, new, parent again — each once under `rocprofv3 --kernel-trace --stats` (the average
# duration of the scoring pass and of smpc_reduce_partials) and once plain (the bench line's ms_per_step).
# The two parent runs of every round are the call's own noise; tools/ab_libs_table.py OUTDIR prints the table.
# Every GPU step runs under its own time limit, and nothing is started after one of them fails.
set -u
A=$1; B=$2; OUT=$3; ROUNDS=${4:-5}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
[ "$(basename "$A")" = libsmpc.so ] && [ "$(basename "$B")" = libsmpc.so ] || { echo "both libraries must be named libsmpc.so"; exit 1; }
A=$(realpath "$A"); B=$(realpath "$B")
mkdir -p "$OUT"
cd "$ROOT"
with_lib() {   # library, command...: the Python side and the compiled loop both on that library
  local lib=$1; shift
  SMPC_LIB=$lib LD_LIBRARY_PATH=$(dirname "$lib")${LD_LIBRARY_PATH:+:$LD_LIBRARY_PATH} "$@"
}
BENCH="python3 bench.py --gpus 1 --steps 200 --warmup 100"
with_lib $A timeout -k 10 300 python3 bench.py --gpus 1 --steps 5 --warmup 2 > /dev/null 2>&1 || exit 1   # (cold host caches)
for r in $(seq 1 "$ROUNDS"); do
  for w in parent:$A new:$B parent2:$A; do
    name=${w%%:*}; lib=${w#*:}
    rm -rf "$OUT/prof"
    with_lib $lib timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- $BENCH \
      > "$OUT/trace_${r}_$name.json" 2> "$OUT/trace_${r}_$name.stderr" || exit 1
    csv=$(find "$OUT/prof" -name "*kernel_stats.csv" | head -1)
    [ -n "$csv" ] || { echo "no kernel_stats.csv from round $r, $name (see $OUT/trace_${r}_$name.stderr)"; exit 1; }
    cp "$csv" "$OUT/kernel_stats_${r}_$name.csv"
    with_lib $lib timeout -k 10 300 $BENCH > "$OUT/bench_${r}_$name.json" 2> "$OUT/bench_${r}_$name.stderr" || exit 1
  done
done
rm -rf "$OUT/prof"
python3 tools/ab_libs_table.py "$OUT" | tee "$OUT/alternating_table.txt"
