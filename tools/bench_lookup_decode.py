#!/usr/bin/env python3
"""What lookup decoding costs and gains (Llama-2-7B Q4_B32T1A synthetic weights, F16 and Q8_B32T2 KV cache, 256 new tokens): one JSON
line per leg.

  --generate KV   through the engine, tokens per second of
                    (a) plain Generate                                            -- the baseline
                    (b) GenerateLookup without a prediction, random prompt        -- acceptance ~ 0: what a miss costs
                    (c) GenerateLookup, prediction = the tokens of the same prompt in the arithmetic a draft step runs (two
                        copies of the query advanced together by Infer / Commit: the batched rows -- with synthetic weights the
                        logits are nearly flat, and the single-row step's int8 activations choose other tokens than the rows'
                        F16 activations, so Generate's own output is NO correct prediction here), at
                        lookup_draft_len 2 / 4 / 7                                -- acceptance ~ 1
                    (d) (c) at draft length 4 with every m-th prediction token corrupted (m = 2, 3, 5, 9, 17): tok/s against
                        the mean accepted tokens per step
                  (a) and the other side alternate inside every repeat; medians.  The ratios (b) / (a) and (c) / (a) are printed.
  --step KV       one ifa_model_decode_draft call at n = 2 / 5 / 8 rows against one ifa_model_decode step, behind ~40 and ~1000 keys
                  (graph replays, wall time around the synchronous call, median of bursts).

KV = f16 | q8.  tools/bench_lookup_decode.sh chains the legs, each under its own time limit."""
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

NEW = 256


def _kv(name):
    from inferflow_amd import dtypes as dt
    return {"f16": dt.F16, "q8": dt.Q8_B32T2}[name]


def engine(d, kv, draft_len):
    from inferflow_amd.engine import InferenceEngine
    text = INI.format(pool="false", model_dir=os.path.join(ROOT, "examples", "llama2_7b_synthetic"))
    text = text.replace("max_concurrent_queries = 8", "max_concurrent_queries = 2\nlookup_draft_len = %d" % draft_len)
    text = text.replace("device_kv_cache_data_type = F16", "device_kv_cache_data_type = %s" % kv.upper())
    ini = os.path.join(d, "bench_sampled.ini")
    open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


def run_generate(kv, repeats):
    rng = np.random.default_rng(7)
    prompt = [int(t) for t in rng.integers(3, 32000, 32)]

    def plain(eng):
        q = eng.add_query(prompt)
        t0 = time.perf_counter()
        toks, _ = eng.generate(q, NEW)
        dt_ = time.perf_counter() - t0
        eng.remove_query(q)
        return toks, NEW / dt_, None

    def lookup(eng, pred):
        q = eng.add_query(prompt)
        t0 = time.perf_counter()
        toks, st = eng.generate_lookup(q, NEW, prediction=pred)
        dt_ = time.perf_counter() - t0
        eng.remove_query(q)
        return toks, NEW / dt_, st

    def rows_truth(eng):
        qa, qb = eng.add_query(prompt), eng.add_query(prompt)
        out = []
        for _ in range(NEW):
            res = dict(eng.infer())
            assert res[qa] == res[qb], "two copies of one query parted in a batched step"
            out.append(res[qa])
            eng.commit({qa: res[qa], qb: res[qb]})
        eng.remove_query(qa); eng.remove_query(qb)
        return out

    def leg(eng, name, pred, extra):
        a, b, st = [], [], None
        plain(eng); lookup(eng, pred)                                   # warm-up: graph captures of every row count
        for _ in range(repeats):                                        # the two sides alternate inside every repeat
            a.append(plain(eng)[1])
            _, r, st = lookup(eng, pred)
            b.append(r)
        ma, mb = float(np.median(a)), float(np.median(b))
        out = {"leg": name, "kv": kv, "new_tokens": NEW, "plain_tok_s": [round(x, 1) for x in a], "plain_tok_s_median": round(ma, 1),
               "lookup_tok_s": [round(x, 1) for x in b], "lookup_tok_s_median": round(mb, 1), "ratio_to_plain": round(mb / ma, 3),
               "stats": st, "tokens_per_step": round(NEW / max(1, st["steps"]), 3)}
        out.update(extra)
        print(json.dumps(out), flush=True)

    with tempfile.TemporaryDirectory() as d:
        for dl in (4, 2, 7):
            eng = engine(d, kv, dl)
            if dl == 4:
                leg(eng, "b_no_prediction", None, {"draft_len": dl})
            truth = rows_truth(eng)
            got = lookup(eng, truth)[0]
            same = next((i for i in range(NEW) if got[i] != truth[i]), NEW)
            print(json.dumps({"leg": "prediction_check", "kv": kv, "draft_len": dl, "leading_tokens_equal_to_prediction": same}), flush=True)
            leg(eng, "c_correct_prediction", truth, {"draft_len": dl})
            if dl == 4:
                for m in (2, 3, 5, 9, 17):
                    bad = [t if (i + 1) % m else (t + 1 if t + 1 < 32000 else 3) for i, t in enumerate(truth)]
                    leg(eng, "d_corrupted_prediction", bad, {"draft_len": dl, "corrupt_every": m})
            eng.close()


def run_step(kv, repeats, burst):
    from inferflow_amd import dtypes as dt, synth
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, _kv(kv), max_ctx=1280)
    rng = np.random.default_rng(9)
    for keys in (40, 1000):
        prompt = rng.integers(3, s["vocab"], keys).astype(np.int32)
        t0 = int(wk.forward(prompt, 0))
        out = {"leg": "step", "kv": kv, "keys": keys}

        def one(fn):
            fn(); fn()
            us = []
            for _ in range(repeats):
                t = time.perf_counter()
                for _ in range(burst):
                    fn()
                us.append(1e6 * (time.perf_counter() - t) / burst)
            return round(float(np.median(us)), 1)

        out["decode_us"] = one(lambda: wk.decode(t0, keys, 1, timed=False))
        for n in (2, 5, 8):
            toks = np.concatenate([[t0], rng.integers(3, s["vocab"], n - 1)]).astype(np.int32)
            out["draft_n%d_us" % n] = one(lambda: wk.decode_draft(toks, keys))
            out["draft_n%d_over_decode" % n] = round(out["draft_n%d_us" % n] / out["decode_us"], 3)
        print(json.dumps(out), flush=True)
    wk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generate", choices=("f16", "q8"), default=None)
    ap.add_argument("--step", choices=("f16", "q8"), default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a.repeats, a.burst)
    if a.generate:
        run_generate(a.generate, a.repeats)


if __name__ == "__main__":
    main()
