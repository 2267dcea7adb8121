#!/usr/bin/env python3
"""Sampled decoding through the Infer / CommitInferenceResult loop (Llama-2-7B Q4_B32T1A synthetic weights, F16 KV cache,
20-token prompt, 128 steps, sample.top_p with a fixed seed, return_output_tensors = false): one JSON line per leg.

  --pool 0   leg 1 (greedy through the same loop: the ceiling of a host-driven loop), leg 2 (sampled, host pool: the logits row
             comes to the host every step -- the path of a build without device_sampling_pool), leg 4 at 8 concurrent queries
  --pool 1   leg 3 (sampled, device_sampling_pool = true) and leg 4 at 8 concurrent queries
  --kernel   leg 5: ifa_topk_pool alone at V = 32000 / 151936, k = 50, rows 1 / 8 (run it under rocprofv3 --kernel-trace --stats)

Every leg is warmed up by one untimed pass and repeated --repeats times (the spread of the repeats is what a difference between
legs has to exceed).  tools/bench_sampled.sh chains the legs, each under its own time limit."""
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

INI = """[main]
inference_engine_config = ${{config_dir}}/bench_sampled.ini

[transformer_engine]
models = llama2_7b_q4
devices = 0
decoder_cpu_layer_count = 0
max_concurrent_queries = 8
return_output_tensors = false
device_sampling_pool = {pool}

[model.llama2_7b_q4]
model_dir = {model_dir}/
model_specification_file = model_spec.json
device_weight_data_type = Q4
device_kv_cache_data_type = F16
max_context_len = 1024
prompt_template = {{bos}}{{query}}
"""


def run_leg(eng, name, strategy, n_queries, steps, repeats, pool):
    rng = np.random.default_rng(3)
    prompts = [[int(t) for t in rng.integers(3, 32000, 20)] for _ in range(n_queries)]
    rates = []
    for rep in range(repeats + 1):                  # pass 0 warms up (graph capture, allocations) and is not reported
        qids = [eng.add_query(p, strategy=strategy, seed=(1234 + i) if strategy else 0) for i, p in enumerate(prompts)]
        assert min(qids) > 0
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
        if rep:
            rates.append(n_queries * steps / dt_s)
    print(json.dumps({"leg": name, "strategy": strategy or "greedy", "device_sampling_pool": bool(pool), "queries": n_queries, "steps": steps,
                      "tok_s": [round(r, 2) for r in rates], "tok_s_median": round(float(np.median(rates)), 2),
                      "ms_per_step_median": round(1e3 * n_queries / float(np.median(rates)), 4),
                      "sampled_fused_steps": eng.model_info("sampled_fused_steps")}), flush=True)


def run_kernel(iters):
    import torch
    from inferflow_amd import worker as W
    for V in (32000, 151936):
        for rows in (1, 8):
            x = torch.from_numpy(np.random.default_rng(V + rows).normal(0, 2.5, (rows, V)).astype(np.float16).view(np.int16)).cuda().view(torch.float16)
            s = torch.cuda.current_stream().cuda_stream
            for _ in range(20):
                W.topk_pool(x, 50, stream=s)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                W.topk_pool(x, 50, stream=s)
            e1.record(); torch.cuda.synchronize()
            print(json.dumps({"leg": "5_pool_kernel", "vocab": V, "rows": rows, "k": 50, "us_per_launch_back_to_back": round(1e3 * e0.elapsed_time(e1) / iters, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=0)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        return run_kernel(a.iters)
    from inferflow_amd.engine import InferenceEngine
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "bench_sampled.ini")
        open(ini, "w").write(INI.format(pool="true" if a.pool else "false", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic")))
        eng = InferenceEngine.from_ini(ini)
        if not a.pool:
            run_leg(eng, "1_greedy_loop", None, 1, a.steps, a.repeats, a.pool)
            run_leg(eng, "2_sampled_host_pool", "sample.top_p", 1, a.steps, a.repeats, a.pool)
            run_leg(eng, "4_sampled_host_pool_x8", "sample.top_p", 8, a.steps, a.repeats, a.pool)
        else:
            run_leg(eng, "3_sampled_device_pool", "sample.top_p", 1, a.steps, a.repeats, a.pool)
            run_leg(eng, "4_sampled_device_pool_x8", "sample.top_p", 8, a.steps, a.repeats, a.pool)
        eng.close()


if __name__ == "__main__":
    main()
