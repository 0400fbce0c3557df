#!/bin/bash
# The committed profile of the bench command itself (default: 1024 blocks resident): a kernel trace with stats, then FETCH_SIZE and
# WRITE_SIZE in counter passes of their own (kernel trace only besides the counter).  tools/save_bench_profile.py turns the output
# into $OUT_DIR/00_bench_command.txt (default build/profb) and profiles/fe_traffic.json, the traffic figure bench.py reports for
# this build.  Run from the repository root on a built tree; stops at the first failing step.
set -eo pipefail
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profb}
rm -rf "$OUT"; mkdir -p "$OUT"
B="python3 bench.py --no-cpu-baseline --no-side-legs"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o trace -- $B --steps 30 --warmup 5 \
    > "$OUT/bench_under_rocprof.log" 2>&1 < /dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE -d "$OUT/pmc_fetch" -o pmc -- $B --steps 5 --warmup 2 --settle-ms 0 \
    > "$OUT/pmc_fetch.log" 2>&1 < /dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE -d "$OUT/pmc_write" -o pmc -- $B --steps 5 --warmup 2 --settle-ms 0 \
    > "$OUT/pmc_write.log" 2>&1 < /dev/null
timeout -k 10 60 python3 tools/save_bench_profile.py "$OUT"
