#!/bin/bash
# The legs of tools/bench_lookup_decode.py, each GPU step under its own time limit, chained: a step that fails ends the run.
#   tools/bench_lookup_decode.sh [log file, default profiles/r10_lookup_decode.log]
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r10_lookup_decode.log}
mkdir -p "$(dirname "$LOG")"
{ echo "# tools/bench_lookup_decode.sh $(date -u +%Y-%m-%dT%H:%MZ): one decode_draft call (n = 2 / 5 / 8) against one decode step at ~40 / ~1000 keys | Generate against GenerateLookup without a prediction, with a correct one (draft length 2 / 4 / 7) and with every m-th token of it corrupted; Llama-2-7B Q4 synthetic, 256 new tokens"; } > "$LOG"
timeout -k 10 300 python tools/bench_lookup_decode.py --step f16 2>&1 | tee -a "$LOG" \
&& timeout -k 10 300 python tools/bench_lookup_decode.py --step q8 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_lookup_decode.py --generate f16 2>&1 | tee -a "$LOG" \
&& timeout -k 10 420 python tools/bench_lookup_decode.py --generate q8 2>&1 | tee -a "$LOG"
