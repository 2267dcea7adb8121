#!/bin/bash
# The legs of tools/bench_logprobs.py, each GPU step under its own time limit, chained: a step that fails ends the run.
#   tools/bench_logprobs.sh [log file, default profiles/r08_logprobs.log] [rocprofv3 output dir, default /tmp/ifa_lse_prof]
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r08_logprobs.log}
PROF=${2:-/tmp/ifa_lse_prof}
mkdir -p "$(dirname "$LOG")" "$PROF"
{ echo "# tools/bench_logprobs.sh $(date -u +%Y-%m-%dT%H:%MZ): perplexity per window (host / device scoring) | decode with logprobs off / on | kernel alone"; } > "$LOG"
timeout -k 10 420 python tools/bench_logprobs.py --ppl 0 2>&1 | tee -a "$LOG" \
&& timeout -k 10 300 python tools/bench_logprobs.py --ppl 1 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_logprobs.py --decode 2>&1 | tee -a "$LOG" \
&& timeout -k 10 120 python tools/bench_logprobs.py --kernel 2>&1 | tee -a "$LOG" \
&& timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$PROF" -o lse -- python tools/bench_logprobs.py --kernel --iters 50 > "$PROF/run.log" 2>&1 \
&& { echo "# rocprofv3 --kernel-trace --stats (tools/bench_logprobs.py --kernel --iters 50): k_lse_rows / k_lse_combine over the three shapes"; \
     head -1 $(find "$PROF" -name "*kernel_stats.csv" | head -1); grep -h "k_lse" $(find "$PROF" -name "*kernel_stats.csv") | head -4; } | tee -a "$LOG"
