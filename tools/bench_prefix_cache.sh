#!/bin/bash
# The legs of tools/bench_prefix_cache.py, each GPU step under its own time limit, chained: a step that fails ends the run.
#   tools/bench_prefix_cache.sh [log file, default profiles/r09_prefix_cache.log]
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r09_prefix_cache.log}
mkdir -p "$(dirname "$LOG")"
{ echo "# tools/bench_prefix_cache.sh $(date -u +%Y-%m-%dT%H:%MZ): ifa_model_kv_copy against 2 * layers hipMemcpyAsync calls (F16 / Q8 cache) | AddQuery -> first token, 1024 shared + 32 new tokens: prefix_cache off / hit in place / hit through the copy"; } > "$LOG"
timeout -k 10 180 python tools/bench_prefix_cache.py --copy f16 2>&1 | tee -a "$LOG" \
&& timeout -k 10 180 python tools/bench_prefix_cache.py --copy q8 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_prefix_cache.py --ttft f16 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_prefix_cache.py --ttft q8 2>&1 | tee -a "$LOG"
