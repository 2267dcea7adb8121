#!/usr/bin/env python3
"""What a context shift costs (Llama-2-7B Q4_B32T1A synthetic weights, max_context_len = 1024, F16 and Q8_B32T2 KV cache): one JSON line
per leg.

  --shift KV     one automatic shift -- ifa_model_kv_shift(slot, keep 4, the plan's discard, 1023 rows) -- next to ifa_model_kv_copy
                 of the same number of moved rows between two slots, in the same process: microseconds per call, enqueued back to back
                 and one at a time (call + synchronise: what the shift adds to the step it precedes).  The worker has the KV geometry
                 of the model (32 layers, kv_dim 4096); its FFN and vocabulary are cut down, neither call sees them.
  --generate KV  tok/s of Generate over 2048 new tokens with context_shift = true, which crosses the limit several times, next to the
                 rate of the last 512 tokens in front of the first shift (wall clock around the calls: the shifts are inside).

  --box          one line that names the box: host name, GPU, its compute units and the library's source hash.

KV = f16 | q8.  Every leg is warmed up and repeated; the repeats are printed, and with them the run-to-run spread (largest minus
smallest repeat) of every figure.  tools/bench_context_shift.sh chains the legs, each
under its own time limit."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.bench_sampled import INI

CTX, KEEP = 1024, 4


def _kv(name):
    from inferflow_amd import dtypes as dt
    return {"f16": dt.F16, "q8": dt.Q8_B32T2}[name]


def run_shift(kv, repeats, burst):
    from inferflow_amd import dtypes as dt, synth
    from inferflow_amd.engine import context_shift_plan
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, _kv(kv), max_ctx=CTX, ffn=256, vocab=1000)
    wk.kv_slots(2)
    rows = CTX - 1
    keep, discard = context_shift_plan(CTX, rows, CTX, KEEP)
    moved = rows - keep - discard
    wk.forward(np.random.default_rng(3).integers(3, 1000, rows).astype(np.int32), 0)      # real rows in slot 0
    rb = dt.row_bytes(_kv(kv), s["kv_heads"] * s["head_dim"])
    nbytes = 2 * s["layers"] * moved * rb

    def shift():
        wk.kv_shift(0, keep, discard, rows)

    def copy():
        wk.kv_copy(0, 1, moved)

    def timed(fn, n, sync_each):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
            if sync_each:
                wk.sync()
        wk.sync()
        return 1e6 * (time.perf_counter() - t0) / n

    out = {"leg": "kv_shift", "kv": kv, "calls_per_repeat": burst, "rows": rows, "keep": keep, "discard": discard, "moved_rows": moved, "segments": 2 * s["layers"],
           "moved_MiB": round(nbytes / 2 ** 20, 1)}
    for fn in (shift, copy):
        timed(fn, 5, False)
    for sync_each, tag in ((False, "back_to_back"), (True, "one_at_a_time")):
        us = {"kv_shift": [], "kv_copy": []}
        for _ in range(repeats):                                        # the two alternate inside every repeat
            for name, fn in (("kv_shift", shift), ("kv_copy", copy)):
                us[name].append(timed(fn, burst, sync_each))
        for name in us:
            med = float(np.median(us[name]))
            out["%s_us_%s" % (name, tag)] = [round(u, 1) for u in us[name]]
            out["%s_us_%s_median" % (name, tag)] = round(med, 1)
            out["%s_us_%s_spread" % (name, tag)] = round(max(us[name]) - min(us[name]), 1)
            out["%s_GB_s_%s" % (name, tag)] = round(nbytes / med / 1e3, 1)
    print(json.dumps(out), flush=True)
    wk.close()


def run_generate(kv, repeats):
    from inferflow_amd.engine import InferenceEngine
    text = INI.format(pool="false", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
    text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = 2\ncontext_shift = true\ncontext_shift_keep = %d" % KEEP)
    text = text.replace("device_kv_cache_data_type = F16", "device_kv_cache_data_type = %s" % kv.upper())
    assert "max_context_len = %d" % CTX in text
    prompt = [int(t) for t in np.random.default_rng(7).integers(3, 32000, 16)]
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "bench_context_shift.ini")
        open(ini, "w").write(text)
        eng = InferenceEngine.from_ini(ini)
        before, across, shifted, shifts = [], [], [], []
        for rep in range(repeats + 1):                                  # the first one warms up (allocations, captured steps)
            q = eng.add_query(prompt)
            eng.generate(q, CTX - len(prompt) - 512)
            t0 = time.perf_counter()
            toks, _ = eng.generate(q, 512)                              # ends at the limit: the last 512 tokens in front of the first shift
            t1 = time.perf_counter()
            assert len(toks) == 512 and eng.query_shifted_tokens(q) == 0
            n0 = eng.model_info("context_shifts")
            more, _ = eng.generate(q, 2048)
            t2 = time.perf_counter()
            assert len(more) == 2048
            if rep:
                before.append(512 / (t1 - t0)); across.append(2048 / (t2 - t1)); shifted.append(eng.query_shifted_tokens(q))
                shifts.append(eng.model_info("context_shifts") - n0)
            eng.remove_query(q)
        print(json.dumps({"leg": "generate", "kv": kv, "max_context_len": CTX, "keep": KEEP, "tok_s_last_512_before_first_shift": [round(x, 1) for x in before],
                          "tok_s_before_median": round(float(np.median(before)), 1), "tok_s_before_spread": round(max(before) - min(before), 1), "tok_s_2048_across_shifts": [round(x, 1) for x in across],
                          "tok_s_across_median": round(float(np.median(across)), 1), "tok_s_across_spread": round(max(across) - min(across), 1),
                          "shifts_per_2048_token_run": shifts, "tokens_dropped_per_run": shifted}), flush=True)
        eng.close()


def run_box():
    import socket
    import torch
    from inferflow_amd import build
    p = torch.cuda.get_device_properties(0)
    print(json.dumps({"leg": "box", "host": socket.gethostname(), "gpu": p.name, "compute_units": p.multi_processor_count, "gpus_used": 1,
                      "source_hash": build.source_hash()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shift", choices=("f16", "q8"), default=None)
    ap.add_argument("--generate", choices=("f16", "q8"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--box", action="store_true")
    ap.add_argument("--burst", type=int, default=200)
    a = ap.parse_args()
    if a.box:
        run_box()
    if a.shift:
        run_shift(a.shift, a.repeats, a.burst)
    if a.generate:
        run_generate(a.generate, min(a.repeats, 3))


if __name__ == "__main__":
    main()
