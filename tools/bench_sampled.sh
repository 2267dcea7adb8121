#!/bin/bash
# The five legs of tools/bench_sampled.py, each GPU step under its own time limit, chained: a step that fails ends the run.
#   tools/bench_sampled.sh [log file, default profiles/r07_sampled_decode.log] [rocprofv3 output dir, default /tmp/ifa_pool_prof]
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r07_sampled_decode.log}
PROF=${2:-/tmp/ifa_pool_prof}
mkdir -p "$(dirname "$LOG")" "$PROF"
{ echo "# tools/bench_sampled.sh $(date -u +%Y-%m-%dT%H:%MZ): legs 1, 2, 4 (host pool) | legs 3, 4 (device pool) | leg 5 (kernel alone)"; } > "$LOG"
timeout -k 10 420 python tools/bench_sampled.py --pool 0 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_sampled.py --pool 1 2>&1 | tee -a "$LOG" \
&& timeout -k 10 120 python tools/bench_sampled.py --kernel 2>&1 | tee -a "$LOG" \
&& timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$PROF" -o pool -- python tools/bench_sampled.py --kernel --iters 50 > "$PROF/run.log" 2>&1 \
&& { echo "# rocprofv3 --kernel-trace --stats (tools/bench_sampled.py --kernel --iters 50): k_topk_pool over all four shapes"; \
     head -1 $(find "$PROF" -name "*kernel_stats.csv" | head -1); grep -h "k_topk_pool" $(find "$PROF" -name "*kernel_stats.csv") | head -3; } | tee -a "$LOG"
