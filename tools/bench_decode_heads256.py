#!/usr/bin/env python3
"""Decode of a Gemma-2B-shaped synthetic model (18 layers, dim 2048, 8 heads over 1 kv head of 256, ffn 16384, every matrix
Q4_B32T1A -- tensor_quant_threshold 0 --, vocabulary 32000, Llama wiring) with ifa_attention_mfma_heads off (the op-by-op step:
fused_supported refuses the head size) and on (the fused, captured step with k_dec_attn256 / the split trio), F16 and Q8_B32T2 caches,
at 32 / 512 / 2048 / 8192 keys (--keys a,b,c: others): tokens per second of 32-step calls that end at that many keys, the two settings
alternating in one process, three windows each by host clock around decode() (which ends in a synchronise), the median window.
Then us per attention launch (ifa_model_time_kernel, event-timed, at that position: k_dec_attn256, or scores + P.V + combine together on
the split route; up to 2048 keys also k_dec_attn256 alone with attn_split_ctx 0), next to the 128-wide k_dec_attn / split trio of a one-layer model with 8 heads over 1 kv head at TWICE the keys:
the same bytes of cache read per head.  The cache holds zeros: the time does not depend on the values."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth

L = ia.lib()
KEYS = [int(a) for a in sys.argv[sys.argv.index("--keys") + 1].split(",")] if "--keys" in sys.argv else [32, 512, 2048, 8192]
STEPS, WINDOWS, WINDOW_S, MAX_CALLS = 32, 3, 0.3, 40
GEMMA_2B = dict(layers=18, dim=2048, heads=8, kv_heads=1, head_dim=256, ffn=16384, vocab=32000)
WIDE128 = dict(layers=1, dim=1024, heads=8, kv_heads=1, head_dim=128, ffn=1024, vocab=1000)


def window(wk, n, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        wk.decode(7, n - STEPS, STEPS)
    return STEPS * calls / (time.perf_counter() - t0)


def main():
    print("cache  keys | off tok/s |  on tok/s | ratio | route on      | attn256 us | one wg us  | 128-wide at 2 x keys us   (windows off / on)", flush=True)
    for kvd, name in ((dt.F16, "F16"), (dt.Q8_B32T2, "Q8")):
        wk, _, _ = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=max(KEYS) + 64, quant_threshold=0, **GEMMA_2B)
        ref, _, _ = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=2 * max(KEYS) + 64, quant_threshold=0, **WIDE128)
        ref.set_option("fuse_attn", 0)
        for n in KEYS:
            calls, tps = {}, {0: [], 1: []}
            for on in (0, 1):               # warm-up (the captured step of this reach), and the calls of a window from one call
                L.ifa_attention_mfma_heads(on)
                assert wk.fused_supported()[0] == bool(on)
                wk.decode(7, n - STEPS, STEPS)
                calls[on] = max(1, min(MAX_CALLS, int(WINDOW_S * window(wk, n, 1) / STEPS)))
            for _ in range(WINDOWS):
                for on in (0, 1):
                    L.ifa_attention_mfma_heads(on)
                    tps[on].append(window(wk, n, calls[on]))
            med = {on: sorted(tps[on])[WINDOWS // 2] for on in (0, 1)}
            L.ifa_attention_mfma_heads(1)
            wk.decode(7, n - 1, 1)                                  # the route of a step at n keys
            r = wk.decode_route()
            wk.set_option("time_pos", n - 1)
            us = wk.time_kernel(1, 200)
            one = us
            if r["kind"] == "split" and n <= 2048:                  # k_dec_attn256 alone at the same keys (attn_split_ctx 0: never split)
                wk.set_option("attn_split_ctx", 0)
                wk.decode(7, n - 1, 1)
                assert wk.decode_route()["kind"] == "one_workgroup"
                one = wk.time_kernel(1, 200)
                wk.set_option("attn_split_ctx", -1)
            ref.decode(7, 2 * n - 1, 1)
            r2 = ref.decode_route()
            ref.set_option("time_pos", 2 * n - 1)
            us2 = ref.time_kernel(1, 200)
            print("%5s %5d | %9.1f | %9.1f | %5.2f | %-13s | %10.1f | %10.1f | %8.1f (%s)   (%s / %s)" % (
                name, n, med[0], med[1], med[1] / med[0], r["kind"] + (" x%d" % r["nsplits"] if r["nsplits"] else ""), us, one, us2, r2["kind"],
                " ".join("%.1f" % t for t in tps[0]), " ".join("%.1f" % t for t in tps[1])), flush=True)
        L.ifa_attention_mfma_heads(0)
        wk.close()
        ref.close()


if __name__ == "__main__":
    main()
