#!/usr/bin/env python3
"""What GenerateBatch buys over the Infer / CommitInferenceResult loop for several concurrent queries (Llama-2-7B Q4_B32T1A
synthetic weights, F16 KV cache, 2 / 8 / 16 / 32 queries, 128 new tokens behind 16-token prompts, greedy and seeded sample.top_p
with device_sampler = true).  One engine, one process: after a warm-up pass of each (graph capture, allocations) the loop and
generate_batch run alternating `--repeats` times; the first new token is the prompt step's on both sides and stays outside the
timed region, which covers the remaining steps.  One JSON line per (queries, strategy): aggregate tokens/s and wall milliseconds
per step of every pass, their medians and run-to-run spread ((max - min) / median), the device milliseconds per step of the batched
rounds (HIP events), and whether the two sides produced the same tokens.

  --feed-only N   N feed launches on 32 rows x 32 layers back to back (run under rocprofv3 --kernel-trace --stats for the kernel's time)"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.bench_sampled import INI


def _queries(eng, prompts, strategy):
    ids = [eng.add_query(p, strategy=strategy, seed=1000 + i) if strategy != "greedy" else eng.add_query(p) for i, p in enumerate(prompts)]
    assert all(q > 0 for q in ids), eng._err()
    return ids


def loop_pass(eng, prompts, strategy, steps):
    ids = _queries(eng, prompts, strategy)
    first = dict(eng.infer())                              # the prompt steps
    eng.commit(first)
    toks = {q: [first[q]] for q in ids}
    gc.collect(); gc.disable()
    t0 = time.perf_counter()
    for _ in range(steps - 1):
        res = dict(eng.infer())
        eng.commit(res)
        for q in ids:
            toks[q].append(res[q])
    dt_s = time.perf_counter() - t0
    gc.enable()
    for q in ids:
        eng.remove_query(q)
    return dt_s, [toks[q] for q in ids], None


def batch_pass(eng, prompts, strategy, steps):
    ids = _queries(eng, prompts, strategy)
    first, _, _ = eng.generate_batch([(q, 1) for q in ids])                # the prompt steps
    gc.collect(); gc.disable()
    t0 = time.perf_counter()
    rest, _, stats = eng.generate_batch([(q, steps - 1) for q in ids])
    dt_s = time.perf_counter() - t0
    gc.enable()
    for q in ids:
        eng.remove_query(q)
    return dt_s, [first[q] + rest[q] for q in ids], stats


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def run(counts, steps, prompt_len, repeats, round_steps):
    from inferflow_amd.engine import InferenceEngine
    rng = np.random.default_rng(3)
    all_prompts = [[int(t) for t in rng.integers(3, 32000, prompt_len)] for _ in range(max(counts))]
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "bench_sampled.ini")
        text = INI.format(pool="true", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
        text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = %d" % max(counts)).replace("max_context_len = 1024", "max_context_len = 256")
        text = text.replace("device_sampling_pool = true", "device_sampling_pool = true\ndevice_sampler = true\nbatch_generate_round_steps = %d" % round_steps)
        open(ini, "w").write(text)
        eng = InferenceEngine.from_ini(ini)
        assert eng.model_info("batch_generate") == 1
        for n in counts:
            prompts = all_prompts[:n]
            for strategy in ("greedy", "sample.top_p"):
                legs = {"loop": [], "generate_batch": []}
                toks, stats = {}, None
                for rep in range(repeats + 1):             # pass 0 warms both up and is not reported
                    for name, fn in (("loop", loop_pass), ("generate_batch", batch_pass)):
                        dt_s, toks[name], st = fn(eng, prompts, strategy, steps)
                        stats = st or stats
                        if rep:
                            legs[name].append(dt_s)
                line = {"queries": n, "strategy": strategy, "new_tokens": steps, "prompt": prompt_len, "round_steps": round_steps, "timed_steps": steps - 1}
                for name, v in legs.items():
                    rates = [n * (steps - 1) / t for t in v]
                    line[name] = {"tok_s": [round(r, 1) for r in rates], "tok_s_median": round(float(np.median(rates)), 1), "spread": spread(rates),
                                  "ms_per_step": [round(1e3 * t / (steps - 1), 4) for t in v], "ms_per_step_median": round(1e3 * float(np.median(v)) / (steps - 1), 4)}
                line["gain"] = round(line["generate_batch"]["tok_s_median"] / line["loop"]["tok_s_median"], 4)
                line["rounds"] = stats["rounds"]
                line["device_ms_per_batched_step"] = round(stats["gpu_ms"] / max(1, stats["batched_steps"] + stats["single_steps"]), 4)
                line["same_tokens"] = toks["loop"] == toks["generate_batch"]
                print(json.dumps(line), flush=True)
        eng.close()


def feed_only(iters):
    import torch
    from inferflow_amd import worker as W
    n, layers = 32, 32
    rows = np.zeros(n, W.BATCH_FEED_ROW)
    rows["live"] = 1
    rows["state_slot"] = -1
    rows["sel"] = -1
    table = np.zeros((layers, n), W.BATCH_ATTN_ROW)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.fields else a).cuda()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    arrays = {"rows": dev(rows), "step": i32(1), "argmax": i32(n) + 7, "tok": i32(n), "pos": i32(n), "attn_rows": dev(table), "ring": i32(256, n),
              "pair_slot": i32(n), "pair_tok": i32(n), "err": i32(1)}
    s = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    done = 0
    e0.record()
    while done < iters:
        for _ in range(min(256, iters - done)):
            W.batch_feed_rows(n, layers, arrays, stream=s)
        done += min(256, iters - done)
        arrays["step"].zero_()
    e1.record(); torch.cuda.synchronize()
    assert int(arrays["err"].item()) == 0
    print(json.dumps({"leg": "feed_kernel", "rows": n, "layers": layers, "launches": iters, "us_per_launch_back_to_back": round(1e3 * e0.elapsed_time(e1) / iters, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="2,8,16,32")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--round-steps", type=int, default=32)
    ap.add_argument("--feed-only", type=int, default=0, metavar="LAUNCHES")
    a = ap.parse_args()
    if a.feed_only:
        return feed_only(a.feed_only)
    run([int(c) for c in a.queries.split(",")], a.steps, a.prompt, a.repeats, a.round_steps)


if __name__ == "__main__":
    main()
