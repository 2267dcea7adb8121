#!/usr/bin/env python3
"""us per call of ifa_attention at head_dim 256 (Gemma-2B: 8 heads over 1 kv head, Gemma-7B: 16 over 16), F16 and Q8_B32T2 caches,
64 / 512 / 2048 queries (--queries a,b,c: others) behind prefix 0: ifa_attention_mfma_heads off (k_attention) and on (the 16-wide tile
kernel at 256) alternating in one process, five windows each between device events, the median window; achieved TFLOP/s with the
switch on (1.5 x 4 n^2 / 2 x 256 x heads flops: the scores twice, P.V once, the causal half).
--model: the two-layer 256-wide synthetic model's 70-token prompt, on against off, by host clock around forward + synchronise."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth
from tests import gpu_util as g
from tests import decode_attn_util as D

L = ia.lib()
WINDOWS, WINDOW_MS, MAX_CALLS = 5, 20.0, 300
QUERIES = [int(a) for a in sys.argv[sys.argv.index("--queries") + 1].split(",")] if "--queries" in sys.argv else [64, 512, 2048]


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / n


def attention():
    print("heads/kv cache queries |  off us |   on us | ratio | TFLOP/s on | max|on - off|", flush=True)
    for heads, kv_heads in ((8, 1), (16, 16)):
        for kvd, name in ((dt.F16, "F16"), (dt.Q8_B32T2, "Q8")):
            for n in QUERIES:
                rng = np.random.default_rng(n + heads)
                q = g.dev(rng.normal(0, 1, (n, heads, 256)).astype(np.float16))
                k = g.dev(D.pack_rows(rng.normal(0, 1, (n, kv_heads * 256)).astype(np.float16), kvd))
                v = g.dev(D.pack_rows(rng.normal(0, 1, (n, kv_heads * 256)).astype(np.float16), kvd))
                outs = {on: g.empty_f16(n, heads * 256) for on in (0, 1)}

                def call(on):
                    L.ifa_attention_mfma_heads(on)
                    ia.check(L.ifa_attention(g.p(q), g.p(k), g.p(v), kvd, n, n, 0, heads, kv_heads, 256, 1.0, 0, 0, heads, g.p(outs[on]), g.stream()))

                calls = {}
                for on in (0, 1):               # warm-up, and the calls of a window from one timed call
                    call(on)
                    torch.cuda.synchronize()
                    calls[on] = max(1, min(MAX_CALLS, int(WINDOW_MS * 1000 / window(lambda: call(on), 1))))
                us = {0: [], 1: []}
                for _ in range(WINDOWS):
                    for on in (0, 1):
                        us[on].append(window(lambda: call(on), calls[on]))
                med = {on: sorted(us[on])[WINDOWS // 2] for on in (0, 1)}
                diff = float((outs[1].float() - outs[0].float()).abs().max())
                tflops = 1.5 * 4 * n * n / 2 * 256 * heads / med[1] / 1e6
                print("%5d/%-2d %5s %7d | %7.1f | %7.1f | %5.1f | %10.1f | %.2g   (windows on: %s)" % (
                    heads, kv_heads, name, n, med[0], med[1], med[0] / med[1], tflops, diff, " ".join("%.1f" % u for u in us[1])), flush=True)
    L.ifa_attention_mfma_heads(0)


def model():
    wk, _, s = synth.build("test_gqa", dt.F16, dt.F16, max_ctx=96, dim=512, heads=2, kv_heads=1, head_dim=256)
    toks = np.random.default_rng(256).integers(3, s["vocab"], 70).astype(np.int32)
    us = {0: [], 1: []}
    for r in range(34):
        for on in (0, 1):
            L.ifa_attention_mfma_heads(on)
            wk.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wk.forward(toks, 0)
            torch.cuda.synchronize()
            if r >= 4:
                us[on].append((time.perf_counter() - t0) * 1e6)
    L.ifa_attention_mfma_heads(0)
    wk.close()
    for on in (0, 1):
        a = sorted(us[on])
        print("model 2 x (2 heads x 256 over 1 kv head), 70-token prompt, switch %d: median %.0f us (%.0f - %.0f), %d runs" % (on, a[len(a) // 2], a[0], a[-1], len(a)), flush=True)


if __name__ == "__main__":
    if "--model" in sys.argv:
        model()
    else:
        attention()
