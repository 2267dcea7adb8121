#!/usr/bin/env python3
"""What the prompt prefix cache costs and saves (Llama-2-7B Q4_B32T1A synthetic weights, F16 and Q8_B32T2 KV cache): one JSON line per leg.

  --copy KV   ifa_model_kv_copy of 128 / 1024 / 4096 rows between two slots against a loop of 2 * layers hipMemcpyAsync
              device-to-device calls (ifa_memcpy_d2d) of the same bytes on the same stream: microseconds per copy and GB/s
              (bytes copied / time; the memory system moves twice that, a read and a write), enqueued back to back and one at a
              time (call + synchronise: what AddQuery's one copy costs end to end).  The worker has the KV geometry of the model
              (32 layers, kv_dim 4096); its FFN and vocabulary are cut down, the copy does not see them.
  --ttft KV   time from AddQuery to the first token (AddQuery + Infer, which ends in a synchronisation) of a 1024-token shared
              prefix + a 32-token suffix through the engine: prefix_cache off (every prompt prefilled from row 0), a hit in place
              (the prefix sits in a free slot), a hit through the copy (it sits in a running query's slot).

KV = f16 | q8.  Every leg is warmed up and repeated; the repeats are printed, the median is what the README quotes.
tools/bench_prefix_cache.sh chains the legs, each under its own time limit."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.bench_sampled import INI

PREFIX, SUFFIX = 1024, 32


def _kv(name):
    from inferflow_amd import dtypes as dt
    return {"f16": dt.F16, "q8": dt.Q8_B32T2}[name]


def run_copy(kv, repeats, burst):
    import inferflow_amd as ia
    from inferflow_amd import dtypes as dt, synth
    L = ia.lib()
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, _kv(kv), max_ctx=4096, ffn=256, vocab=1000)
    wk.kv_slots(2)
    layers, rb = s["layers"], dt.row_bytes(_kv(kv), s["kv_heads"] * s["head_dim"])
    ptrs = []
    for slot in (0, 1):
        wk.select_kv(slot)
        ptrs.append([wk.buffer(n, l)[0] for l in range(layers) for n in ("kcache", "vcache")])
    stream = C.c_void_p(L.ifa_model_stream(wk._h))

    def kernel(rows):
        wk.kv_copy(0, 1, rows)

    def memcpy_loop(rows):
        for src, dst in zip(*ptrs):
            ia.check(L.ifa_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), rows * rb, stream))

    def timed(fn, rows, n, sync_each):
        t0 = time.perf_counter()
        for _ in range(n):
            fn(rows)
            if sync_each:
                wk.sync()
        wk.sync()
        return 1e6 * (time.perf_counter() - t0) / n

    for rows in (128, 1024, 4096):
        nbytes = 2 * layers * rows * rb
        out = {"leg": "kv_copy", "kv": kv, "rows": rows, "segments": 2 * layers, "MiB": round(nbytes / 2 ** 20, 1)}
        for name, fn in (("kernel", kernel), ("memcpy_loop", memcpy_loop)):
            timed(fn, rows, 5, False)                                   # warm-up
        for sync_each, tag in ((False, "back_to_back"), (True, "one_at_a_time")):
            us = {"kernel": [], "memcpy_loop": []}
            for _ in range(repeats):                                    # the two alternate inside every repeat
                for name, fn in (("kernel", kernel), ("memcpy_loop", memcpy_loop)):
                    us[name].append(timed(fn, rows, burst, sync_each))
            for name in us:
                med = float(np.median(us[name]))
                out["%s_us_%s" % (name, tag)] = [round(u, 1) for u in us[name]]
                out["%s_us_%s_median" % (name, tag)] = round(med, 1)
                out["%s_GB_s_%s" % (name, tag)] = round(nbytes / med / 1e3, 1)
        out["kernel_faster_back_to_back"] = out["kernel_us_back_to_back_median"] < out["memcpy_loop_us_back_to_back_median"]
        out["kernel_faster_one_at_a_time"] = out["kernel_us_one_at_a_time_median"] < out["memcpy_loop_us_one_at_a_time_median"]
        print(json.dumps(out), flush=True)
    wk.close()


def engine(d, kv, on):
    from inferflow_amd.engine import InferenceEngine
    text = INI.format(pool="false", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
    text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = 2\nprefix_cache = %s" % ("true" if on else "false"))
    text = text.replace("device_kv_cache_data_type = F16", "device_kv_cache_data_type = %s" % kv.upper())
    text = text.replace("max_context_len = 1024", "max_context_len = 1280")
    ini = os.path.join(d, "bench_sampled.ini")
    open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


def run_ttft(kv, repeats):
    rng = np.random.default_rng(7)
    shared = [int(t) for t in rng.integers(3, 32000, PREFIX)]

    def tail(n=SUFFIX):
        return [int(t) for t in rng.integers(3, 32000, n)]

    def first_token(eng, prompt, expect_cached):
        t0 = time.perf_counter()
        q = eng.add_query(prompt)
        res = eng.infer()
        ms = 1e3 * (time.perf_counter() - t0)
        assert q > 0 and any(i == q for i, _ in res), (q, res)
        assert eng.query_cached_tokens(q) == expect_cached, (eng.query_cached_tokens(q), expect_cached)
        return q, ms

    def report(way, ms, eng):
        print(json.dumps({"leg": "first_token", "kv": kv, "way": way, "prefix": PREFIX, "suffix": SUFFIX, "ms": [round(m, 3) for m in ms],
                          "ms_median": round(float(np.median(ms)), 3), "prefix_cache": eng.prefix_cache_stats()}), flush=True)

    with tempfile.TemporaryDirectory() as d:
        eng = engine(d, kv, on=False)
        ms = []
        for rep in range(repeats + 2):                                  # the first two warm up (allocations, code objects)
            q, t = first_token(eng, shared + tail(), 0)
            eng.remove_query(q)
            if rep >= 2:
                ms.append(t)
        report("off", ms, eng)
        eng.close()
        eng = engine(d, kv, on=True)
        q, _ = first_token(eng, shared + tail(), 0)                     # leaves the prefix's rows in a free slot
        eng.remove_query(q)
        ms = []
        for rep in range(repeats + 2):
            q, t = first_token(eng, shared + tail(), PREFIX)
            eng.remove_query(q)
            if rep >= 2:
                ms.append(t)
        report("hit_in_place", ms, eng)
        holder, _ = first_token(eng, shared + tail(), PREFIX)           # stays active: from here the prefix sits in a busy slot
        ms = []
        for rep in range(repeats + 2):
            q, t = first_token(eng, shared + tail(), PREFIX)
            eng.remove_query(q)
            scrub, _ = first_token(eng, tail(64), 0)                    # the freed slot forgets the prefix: the next hit copies again
            eng.remove_query(scrub)
            if rep >= 2:
                ms.append(t)
        report("hit_through_copy", ms, eng)
        assert eng.model_info("prefix_cache_copies") == repeats + 2
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copy", choices=("f16", "q8"), default=None)
    ap.add_argument("--ttft", choices=("f16", "q8"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if a.copy:
        run_copy(a.copy, a.repeats, a.burst)
    if a.ttft:
        run_ttft(a.ttft, a.repeats)


if __name__ == "__main__":
    main()
