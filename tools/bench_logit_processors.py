#!/usr/bin/env python3
"""What the logit processors cost (Llama-2-7B Q4_B32T1A synthetic weights, F16 KV cache, 20-token prompt, 128 steps, sample.top_p on
the device pool with a fixed seed, Infer / CommitInferenceResult loop): one JSON line per leg.

  (default)  batch 1 and batch 8, each WITHOUT processors and WITH frequency_penalty = 0.5; the two sides alternate inside every
             repeat (the spread of the repeats is what a difference has to exceed); tok/s per repeat and medians, their ratio
  --kernel   ifa_logit_adjust_rows alone at V = 32000 / 151936, rows 1 / 8, back to back (run it under
             rocprofv3 --kernel-trace --stats for the kernel's own time; the yardstick is ifa_logsumexp_rows, 5.5 us for one
             32000-id row: the adjust kernel moves about 6 x that row's bytes)"""
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


def one_pass(eng, prompts, steps, opts):
    qids = [eng.add_query(p, strategy="sample.top_p", seed=1234 + i, **opts) for i, p in enumerate(prompts)]
    assert min(qids) > 0, eng._err()
    res = dict(eng.infer())                     # the prompt steps
    eng.commit(res)
    gc.collect(); gc.disable()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = dict(eng.infer())
        eng.commit(res)
    dt_s = time.perf_counter() - t0
    gc.enable()
    for q in qids:
        eng.remove_query(q)
    return len(prompts) * steps / dt_s


def run_engine(steps, repeats):
    from inferflow_amd.engine import InferenceEngine
    rng = np.random.default_rng(3)
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "bench_sampled.ini")
        open(ini, "w").write(INI.format(pool="true", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic")))
        eng = InferenceEngine.from_ini(ini)
        for n in (1, 8):
            prompts = [[int(t) for t in rng.integers(3, 32000, 20)] for _ in range(n)]
            one_pass(eng, prompts, steps, {}); one_pass(eng, prompts, steps, {"frequency_penalty": 0.5})      # warm-up: captures, allocations
            plain, proc = [], []
            for _ in range(repeats):
                plain.append(one_pass(eng, prompts, steps, {}))
                proc.append(one_pass(eng, prompts, steps, {"frequency_penalty": 0.5}))
            mp, mq = float(np.median(plain)), float(np.median(proc))
            print(json.dumps({"leg": "engine", "queries": n, "steps": steps, "plain_tok_s": [round(x, 1) for x in plain], "plain_tok_s_median": round(mp, 1),
                              "processed_tok_s": [round(x, 1) for x in proc], "processed_tok_s_median": round(mq, 1), "ratio": round(mq / mp, 4),
                              "us_per_step_added": round(1e6 * n * (1 / mq - 1 / mp), 2), "processed_steps": eng.model_info("processed_steps")}), flush=True)
        eng.close()


def run_kernel(iters):
    import torch
    from inferflow_amd import worker as W
    for V in (32000, 151936):
        for rows in (1, 8):
            rng = np.random.default_rng(V + rows)
            x = torch.from_numpy(rng.normal(0, 2.5, (rows, V)).astype(np.float16).view(np.int16)).cuda().view(torch.float16)
            state = torch.from_numpy(rng.integers(0, 3, (rows, V)).astype(np.int32)).cuda()
            bias = torch.zeros((rows, V), dtype=torch.float32, device="cuda")
            params = torch.tensor([[1.0, 0.5, 0.0]] * rows, dtype=torch.float32, device="cuda")
            slots = torch.arange(rows, dtype=torch.int32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            for _ in range(20):
                W.logit_adjust_rows(x, slots, state, bias, params, stream=s)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                W.logit_adjust_rows(x, slots, state, bias, params, stream=s)
            e1.record(); torch.cuda.synchronize()
            print(json.dumps({"leg": "adjust_kernel", "vocab": V, "rows": rows, "bytes_moved": rows * V * 12,
                              "us_per_launch_back_to_back": round(1e3 * e0.elapsed_time(e1) / iters, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        return run_kernel(a.iters)
    run_engine(a.steps, a.repeats)


if __name__ == "__main__":
    main()
