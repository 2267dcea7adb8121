#!/usr/bin/env python3
"""What lookup decoding gains and costs for a seeded SAMPLED query (`lookup_sampled = true`; Llama-2-7B Q4_B32T1A synthetic weights,
F16 KV cache, sample.top_p with a fixed seed, 256 new tokens behind a 32-token prompt): one JSON line per leg.

  --generate   through the engine, wall-clock tokens per second of Generate() with device_sampler (the baseline) against
               GenerateLookup, the two alternating inside every repeat, at lookup_draft_len 4 / 2 / 7:
                 no_prediction     GenerateLookup without a prediction (draft length 4 only): what a miss costs
                 first_run         prediction = the tokens of a first GenerateLookup run of the same seeded query.  With synthetic
                                   weights the logits are nearly flat: the first run's plain steps (single row, int8 activations) and
                                   the rows of a draft step (F16 activations) draw other tokens from the same generator stream, so
                                   this prediction goes wrong early and the acceptance stays low
                 rows_truth        prediction = the query's tokens in the arithmetic a draft step runs (two-row draft steps with a
                                   junk draft on the engine's worker, token for token): the prediction is right, acceptance ~ 1
               Acceptance = accepted / drafted draft tokens.
  --step       one ifa_model_decode_draft_sampled call of 5 rows against one ifa_model_decode_draft call of 5 rows behind ~40 keys
               (graph replays, wall time around the synchronous call, median of bursts), without and with logit processors
  --kernel     back-to-back launches timed with events, `--repeats` groups of `--iters`: ifa_sample_verify_rows at 5 rows / pool 50
               against ifa_sample_pool_rows on the same 5 pools; ifa_logit_adjust_draft_rows against ifa_logit_adjust_rows for 5 rows
               of 32000 ids"""
import argparse
import ctypes as C
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

NEW, SEED, STRATEGY = 256, 1234, "sample.top_p"
MAX_K, TOP_P, MIN_P, POOL = 8, 0.9, 0.05, 50           # host/sampling_strategy.h: SamplingConfig


def engine(d, draft_len):
    from inferflow_amd.engine import InferenceEngine
    text = INI.format(pool="true", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
    text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = 2\ndevice_sampler = true\nlookup_sampled = true\nlookup_draft_len = %d" % draft_len)
    ini = os.path.join(d, "bench_sampled.ini")
    open(ini, "w").write(text)
    eng = InferenceEngine.from_ini(ini)
    assert eng.model_info("lookup_sampled") == 1
    return eng


def rows_truth(eng, prompt):
    """the seeded query's tokens with every step a two-row draft step (junk draft) on the engine's worker: the draft rows' arithmetic"""
    import inferflow_amd as ia
    from inferflow_amd import _capi, worker as W

    class Borrowed(W.DecodeWorker):
        def __init__(self, h):
            self._h = C.c_void_p(h)

        def close(self):
            pass

    q = eng.add_query(prompt, strategy=STRATEGY, seed=SEED)
    toks, _ = eng.generate(q, 1)
    st = eng.query_rng_state(q)
    wk = Borrowed(ia.lib().ifa_engine_worker(eng._h, 0))
    p = _capi.SampleParams(eng.strategy_id(STRATEGY), 1.0, TOP_P, MAX_K, MIN_P, POOL)
    pos = len(prompt)
    while len(toks) < NEW:
        out, st = wk.decode_draft_sampled([toks[-1], 3], pos, p, st)
        toks += [int(t) for t in out]
        pos += len(out)
    eng.remove_query(q)
    return toks[:NEW]


def run_generate(repeats):
    prompt = [int(t) for t in np.random.default_rng(7).integers(3, 32000, 32)]

    def timed(eng, fn):
        q = eng.add_query(prompt, strategy=STRATEGY, seed=SEED)
        assert q > 0, eng._err()
        gc.collect(); gc.disable()
        t0 = time.perf_counter()
        toks, st = fn(q)
        dt_ = time.perf_counter() - t0
        gc.enable()
        eng.remove_query(q)
        return toks, NEW / dt_, st

    def plain(eng):
        return timed(eng, lambda q: eng.generate(q, NEW))

    def lookup(eng, pred):
        return timed(eng, lambda q: eng.generate_lookup(q, NEW, prediction=pred))

    def leg(eng, name, pred, dl):
        a, b, st, toks = [], [], None, None
        plain(eng); lookup(eng, pred)                                   # warm-up: graph captures of every row count
        for _ in range(repeats):                                        # the two sides alternate inside every repeat
            a.append(plain(eng)[1])
            toks, r, st = lookup(eng, pred)
            b.append(r)
        ma, mb = float(np.median(a)), float(np.median(b))
        same = next((i for i in range(min(NEW, len(pred))) if toks[i] != pred[i]), min(NEW, len(pred))) if pred else None
        print(json.dumps({"leg": name, "draft_len": dl, "new_tokens": NEW, "generate_tok_s": [round(x, 1) for x in a], "generate_tok_s_median": round(ma, 1),
                          "lookup_tok_s": [round(x, 1) for x in b], "lookup_tok_s_median": round(mb, 1), "ratio_to_generate": round(mb / ma, 3),
                          "stats": st, "acceptance": round(st["accepted"] / max(1, st["drafted"]), 3), "tokens_per_step": round(NEW / max(1, st["steps"]), 3),
                          "leading_tokens_equal_to_prediction": same}), flush=True)

    with tempfile.TemporaryDirectory() as d:
        for dl in (4, 2, 7):
            eng = engine(d, dl)
            if dl == 4:
                leg(eng, "no_prediction", None, dl)
            leg(eng, "first_run", lookup(eng, None)[0], dl)
            leg(eng, "rows_truth", rows_truth(eng, prompt), dl)
            eng.close()


def run_step(repeats, burst):
    from inferflow_amd import _capi, dtypes as dt, synth, worker as W
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, dt.F16, max_ctx=1280)
    rng = np.random.default_rng(9)
    keys, n = 40, 5
    prompt = rng.integers(3, s["vocab"], keys).astype(np.int32)
    t0 = int(wk.forward(prompt, 0))
    toks = np.concatenate([[t0], rng.integers(3, s["vocab"], n - 1)]).astype(np.int32)
    p = _capi.SampleParams(4, 1.0, TOP_P, MAX_K, MIN_P, POOL)
    wk.logit_state_reset(0, prompt, rep=1.3, freq=0.25, pres=0.5)
    st0 = W.rng_state_of_seed(SEED)

    def one(fn):
        fn(); fn()
        us = []
        for _ in range(repeats):
            t = time.perf_counter()
            for _ in range(burst):
                fn()
            us.append(1e6 * (time.perf_counter() - t) / burst)
        return round(float(np.median(us)), 1), round(float(min(us)), 1), round(float(max(us)), 1)

    out = {"leg": "step", "keys": keys, "rows": n, "pool": POOL}
    for name, fn in (("draft_us", lambda: wk.decode_draft(toks, keys)),
                     ("draft_sampled_us", lambda: wk.decode_draft_sampled(toks, keys, p, st0)),
                     ("draft_sampled_processed_us", lambda: wk.decode_draft_sampled(toks, keys, p, st0, 0)),
                     ("draft_again_us", lambda: wk.decode_draft(toks, keys))):
        out[name], out[name + "_min"], out[name + "_max"] = one(fn)
    out["sampled_minus_draft_us"] = round(out["draft_sampled_us"] - out["draft_us"], 1)
    out["processed_minus_draft_us"] = round(out["draft_sampled_processed_us"] - out["draft_us"], 1)
    print(json.dumps(out), flush=True)
    wk.close()


def run_kernel(repeats, iters):
    import torch
    from inferflow_amd import worker as W
    from tests.pool_util import pool_ref
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def groups(fn):
        fn(); torch.cuda.synchronize()
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / iters)
        return {"us_per_launch_median": round(float(np.median(us)), 2), "us_per_launch_min": round(min(us), 2), "us_per_launch_max": round(max(us), 2)}

    rows, k = 5, 50
    pools = [pool_ref(rng.normal(0, 0.06, 32000).astype(np.float16), k) for _ in range(rows)]
    counts = dev(np.full(rows, k, np.int32))
    ids = dev(np.stack([i for i, _ in pools]))
    vals = dev(np.stack([b for _, b in pools]).view(np.int16))
    par1 = W.sample_params_array([(4, 1.0, TOP_P, MAX_K, MIN_P)])
    # drafts that the chain accepts: all 5 rows are walked
    st, draft = W.rng_state_of_seed(1), []
    for i, b in pools[:-1]:
        tok, _, _, _, _, st = W.sample_pool_host(i, b, par1[0], st)
        draft.append(tok)
    params1, params5 = dev(par1.view(np.uint8).copy()), dev(W.sample_params_array([(4, 1.0, TOP_P, MAX_K, MIN_P)] * rows).view(np.uint8).copy())
    draft_d = dev(np.array(draft, np.int32))
    rng1, rng5 = dev(np.array([W.rng_state_of_seed(1)], np.int64)), dev(np.array([W.rng_state_of_seed(1)] * rows, np.int64))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for name, fn in (("ifa_sample_pool_rows", lambda: W.sample_pool_rows(counts, ids, vals, params5, rng5, err, stream=s)),
                     ("ifa_sample_verify_rows", lambda: W.sample_verify_rows(counts, ids, vals, params1, draft_d, rng1, err, want_index=False, stream=s)),
                     ("ifa_sample_pool_rows_again", lambda: W.sample_pool_rows(counts, ids, vals, params5, rng5, err, stream=s))):
        print(json.dumps(dict({"leg": "kernel", "op": name, "rows": rows, "pool": k, "launches": iters, "groups": repeats}, **groups(fn))), flush=True)
    assert int(err.item()) == 0

    V = 32000
    lg = dev(rng.normal(0, 2.0, (rows, V)).astype(np.float16))
    state = dev(rng.choice(np.array([0, 1, 7], np.int32), (1, V)))
    bias = torch.zeros((1, V), dtype=torch.float32, device="cuda")
    par = dev(np.array([[1.3, 0.25, 0.5]], np.float32))
    slots5, slot1 = torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for name, fn in (("ifa_logit_adjust_rows", lambda: W.logit_adjust_rows(lg, slots5, state, bias, par, stream=s)),
                     ("ifa_logit_adjust_draft_rows", lambda: W.logit_adjust_draft_rows(lg, slot1, draft_d, state, bias, par, stream=s)),
                     ("ifa_logit_adjust_rows_again", lambda: W.logit_adjust_rows(lg, slots5, state, bias, par, stream=s))):
        print(json.dumps(dict({"leg": "kernel", "op": name, "rows": rows, "vocab": V, "launches": iters, "groups": repeats}, **groups(fn))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        run_kernel(max(a.repeats, 5), a.iters)
    if a.step:
        run_step(max(a.repeats, 5), a.burst)
    if a.generate:
        run_generate(a.repeats)


if __name__ == "__main__":
    main()
