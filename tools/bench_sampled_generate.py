#!/usr/bin/env python3
"""What the device sampler buys (Llama-2-7B Q4_B32T1A synthetic weights, F16 KV cache, one sample.top_p query with a fixed seed,
256 new tokens behind a 21-token prompt): one JSON line per leg, wall-clock tokens/s of the 256 steps behind the prompt step.

  --mode loop      the Infer / CommitInferenceResult loop with device_sampling_pool = true (one synchronisation per token)
  --mode generate  Generate() with device_sampler = true (the replayed graph draws on the device)
  --kernel         ifa_sample_pool_rows alone, one row, pool 50 / 256, with and without equal values, `--iters` launches each in
                   this order (run it under rocprofv3 --kernel-trace for the kernel's own time per group of launches)

Each mode runs the query WITHOUT processors and WITH frequency_penalty = 0.5, a warm-up pass (graph capture, allocations) in front
of every timed one.  IFA_LIB=<another build's libinferflow_amd.so> runs the loop on that library (--tag names it in the line)."""
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


def loop_pass(eng, prompt, steps, opts):
    q = eng.add_query(prompt, strategy="sample.top_p", seed=1234, **opts)
    assert q > 0, eng._err()
    eng.commit(dict(eng.infer()))                   # the prompt step
    gc.collect(); gc.disable()
    t0 = time.perf_counter()
    toks = []
    for _ in range(steps):
        res = dict(eng.infer())
        eng.commit(res)
        toks.append(res[q])
    dt_s = time.perf_counter() - t0
    gc.enable()
    eng.remove_query(q)
    return steps / dt_s, toks


def generate_pass(eng, prompt, steps, opts):
    q = eng.add_query(prompt, strategy="sample.top_p", seed=1234, **opts)
    assert q > 0, eng._err()
    eng.generate(q, 1)                              # the prompt step
    gc.collect(); gc.disable()
    t0 = time.perf_counter()
    toks, gpu_ms = eng.generate(q, steps)
    dt_s = time.perf_counter() - t0
    gc.enable()
    eng.remove_query(q)
    return steps / dt_s, toks, gpu_ms


def run_engine(mode, steps, prompt_len, repeats, tag):
    from inferflow_amd.engine import InferenceEngine
    prompt = [int(t) for t in np.random.default_rng(3).integers(3, 32000, prompt_len)]
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "bench_sampled.ini")
        text = INI.format(pool="true", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
        if mode == "generate":
            text = text.replace("device_sampling_pool = true", "device_sampling_pool = true\ndevice_sampler = true")
        open(ini, "w").write(text)
        eng = InferenceEngine.from_ini(ini)
        for name, opts in (("plain", {}), ("frequency_penalty_0.5", {"frequency_penalty": 0.5})):
            rates, toks, gpu = [], None, None
            for rep in range(repeats + 1):          # pass 0 warms up and is not reported
                if mode == "loop":
                    r, toks = loop_pass(eng, prompt, steps, opts)
                else:
                    r, toks, gpu = generate_pass(eng, prompt, steps, opts)
                if rep:
                    rates.append(round(r, 1))
            line = {"leg": mode, "lib": tag, "query": name, "steps": steps, "prompt": prompt_len, "tok_s": rates,
                    "tok_s_median": float(np.median(rates)), "last_tokens": toks[-4:]}
            if gpu is not None:
                line["gpu_event_ms_per_step"] = round(gpu / steps, 4)
                line["device_sampled_steps"] = eng.model_info("device_sampled_steps")
            print(json.dumps(line), flush=True)
        eng.close()


def run_kernel(iters):
    import torch
    from inferflow_amd import worker as W
    from tests.pool_util import pool_ref
    rng = np.random.default_rng(5)
    for k in (50, 256):
        for ties in (False, True):
            if ties:
                row = rng.normal(0, 0.06, 32000).astype(np.float16)             # F16 logits of a model's scale: equal values by themselves
            else:
                row = np.unique(rng.normal(0, 2.0, 32000).astype(np.float16))
                rng.shuffle(row)
            ids, bits = pool_ref(row, k)
            if ties:
                bits = bits.copy()
                bits[2::3] = bits[1::3][:bits[2::3].size]                        # and every third entry equal to the one before it
            v = bits.view(np.float16).astype(np.float32)
            n_equal = int(np.sum(v[1:] == v[:-1]))
            assert (n_equal > 0) == ties
            dev = lambda a: torch.from_numpy(a).cuda()
            counts, ids_d, vals_d = dev(np.array([k], np.int32)), dev(ids.reshape(1, k).copy()), dev(bits.view(np.int16).reshape(1, k).copy())
            params = dev(W.sample_params_array([(4, 1.0, 0.9, 8, 0.05)]).view(np.uint8).copy())
            states = dev(np.array([W.rng_state_of_seed(1)], np.int64))
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                W.sample_pool_rows(counts, ids_d, vals_d, params, states, err, stream=s)
            e1.record(); torch.cuda.synchronize()
            print(json.dumps({"leg": "sample_kernel", "pool": k, "equal_neighbours": n_equal, "launches": iters,
                              "us_per_launch_back_to_back": round(1e3 * e0.elapsed_time(e1) / iters, 2)}), flush=True)


def summarise(path, iters):
    """the kernel's own time per group of `iters` launches from a rocprofv3 --kernel-trace CSV of `--kernel --iters N`"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "k_sample_pool" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = ["pool 50", "pool 50, equal values", "pool 256", "pool 256, equal values"]
    assert len(rows) == iters * len(names), (len(rows), iters)
    for g, name in enumerate(names):
        ns = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[g * iters:(g + 1) * iters]], np.float64)
        print(json.dumps({"leg": "sample_kernel_trace", "group": name, "launches": iters, "us_mean": round(float(ns.mean()) / 1e3, 2),
                          "us_median": round(float(np.median(ns)) / 1e3, 2), "us_min": round(float(ns.min()) / 1e3, 2),
                          "us_max": round(float(ns.max()) / 1e3, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["loop", "generate"], default="generate")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="per-group kernel times from the trace of a --kernel run with the same --iters")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.iters)
    if a.kernel:
        return run_kernel(a.iters)
    run_engine(a.mode, a.steps, a.prompt, a.repeats, a.tag)


if __name__ == "__main__":
    main()
