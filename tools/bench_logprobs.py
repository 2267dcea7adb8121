#!/usr/bin/env python3
"""What log-probabilities cost (Llama-2-7B Q4_B32T1A synthetic weights, F16 KV cache): one JSON line per leg.

  --ppl S     perplexity harness over 8 windows of 512 tokens: wall time per window, device scoring off (S = 0: the logits block comes
              to the host, return_output_tensors = true) or on (S = 1: ScoreTokens, return_output_tensors = false)
  --decode    Infer / Commit loop, 128 steps, greedy and sample.top_p (device_sampling_pool = true), logprobs off (-1) and on (5)
  --kernel    ifa_logsumexp_rows alone at 1 x 32000, 1 x 151936, 512 x 32000 (run it under rocprofv3 --kernel-trace --stats)

tools/bench_logprobs.sh chains the legs, each under its own time limit."""
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


def engine(d, ret, pool=True, maxq=2):
    from inferflow_amd.engine import InferenceEngine
    text = INI.format(pool="true" if pool else "false", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
    text = text.replace("return_output_tensors = false", "return_output_tensors = %s" % ("true" if ret else "false"))
    text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = %d" % maxq)
    ini = os.path.join(d, "bench_sampled.ini")
    open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


def run_ppl(device_scoring, windows, repeats):
    toks = [int(t) for t in np.random.default_rng(11).integers(3, 32000, 512 * windows)]
    with tempfile.TemporaryDirectory() as d:
        eng = engine(d, ret=not device_scoring, maxq=1)
        times = []
        for rep in range(repeats + 1):              # pass 0 warms up
            t0 = time.perf_counter()
            ppl, err, count = eng.perplexity(toks, max_length=512, stride=512, device_scoring=bool(device_scoring))
            if rep:
                times.append((time.perf_counter() - t0) / windows)
        eng.close()
    print(json.dumps({"leg": "perplexity", "device_scoring": bool(device_scoring), "windows": windows, "tokens_per_window": 512,
                      "ms_per_window": [round(1e3 * t, 3) for t in times], "ms_per_window_median": round(1e3 * float(np.median(times)), 3),
                      "ppl": ppl, "count": count}), flush=True)


def run_decode(steps, repeats):
    prompt = [int(t) for t in np.random.default_rng(3).integers(3, 32000, 20)]
    with tempfile.TemporaryDirectory() as d:
        eng = engine(d, ret=False, pool=True)
        for strategy in (None, "sample.top_p"):
            for lp in (-1, 5):
                rates = []
                for rep in range(repeats + 1):
                    q = eng.add_query(prompt, strategy=strategy, seed=1234 if strategy else 0, logprobs=lp)
                    assert q > 0
                    eng.commit(dict(eng.infer()))
                    gc.collect(); gc.disable()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        eng.commit(dict(eng.infer()))
                    dt_s = time.perf_counter() - t0
                    gc.enable()
                    eng.remove_query(q)
                    if rep:
                        rates.append(steps / dt_s)
                print(json.dumps({"leg": "decode", "strategy": strategy or "greedy", "logprobs": lp, "steps": steps, "tok_s": [round(r, 2) for r in rates],
                                  "tok_s_median": round(float(np.median(rates)), 2), "ms_per_step_median": round(1e3 / float(np.median(rates)), 4)}), flush=True)
        eng.close()


def run_kernel(iters):
    import torch
    from inferflow_amd import worker as W
    for rows, V in ((1, 32000), (1, 151936), (512, 32000)):
        x = torch.from_numpy(np.random.default_rng(V + rows).normal(0, 2.5, (rows, V)).astype(np.float16).view(np.int16)).cuda().view(torch.float16)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(20):
            W.logsumexp_rows(x, stream=s)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            W.logsumexp_rows(x, stream=s)
        e1.record(); torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / iters
        print(json.dumps({"leg": "lse_kernel", "vocab": V, "rows": rows, "us_per_call_back_to_back": round(us, 2),
                          "GB_s": round(rows * V * 2 / us / 1e3, 1), "of_8TB_s": round(rows * V * 2 / us / 1e3 / 8000, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ppl", type=int, default=None)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        run_kernel(a.iters)
    if a.ppl is not None:
        run_ppl(a.ppl, a.windows, a.repeats)
    if a.decode:
        run_decode(a.steps, a.repeats)


if __name__ == "__main__":
    main()
