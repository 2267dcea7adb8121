#!/bin/bash
# The legs of tools/bench_context_shift.py, each GPU step under its own time limit, chained: a step that fails ends the run.
#   tools/bench_context_shift.sh [log file, default profiles/r14_context_shift.log]
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r14_context_shift.log}
mkdir -p "$(dirname "$LOG")"
{ echo "# tools/bench_context_shift.sh $(date -u +%Y-%m-%dT%H:%MZ): one automatic shift (keep 4, 1023 rows) against ifa_model_kv_copy of the moved rows (F16 / Q8 cache) | Generate over 2048 tokens across the limit against the last 512 tokens in front of the first shift, Llama-2-7B Q4, max_context_len 1024.  First line below: the box.  Every leg lists its repeats and their run-to-run spread (*_spread: largest minus smallest repeat)."; } > "$LOG"
timeout -k 10 120 python tools/bench_context_shift.py --box 2> >(grep -v amdgpu.ids >&2) | tee -a "$LOG" \
&& timeout -k 10 180 python tools/bench_context_shift.py --shift f16 2> >(grep -v amdgpu.ids >&2) | tee -a "$LOG" \
&& timeout -k 10 180 python tools/bench_context_shift.py --shift q8 2> >(grep -v amdgpu.ids >&2) | tee -a "$LOG" \
&& timeout -k 10 300 python tools/bench_context_shift.py --generate f16 2> >(grep -v amdgpu.ids >&2) | tee -a "$LOG" \
&& timeout -k 10 300 python tools/bench_context_shift.py --generate q8 2> >(grep -v amdgpu.ids >&2) | tee -a "$LOG"
