#!/usr/bin/env python3
"""Batched decode steps of a Gemma-2B-shaped synthetic model (18 layers, dim 2048, 8 heads over 1 kv head of 256, ffn 16384, every
matrix Q4_B32T1A -- tensor_quant_threshold 0 --, vocabulary 32000, Llama wiring): decode_batch of 2 / 8 / 16 / 32 rows that end at
32 / 512 / 2048 keys (--rows a,b / --keys a,b: others), F16 and Q8_B32T2 caches, ifa_attention_mfma_heads at level 0 (op by op:
k_attention, one workgroup per (head, row)) and level 2 (the fused, captured step with k_dec_attn256_batch) alternating in one
process, three windows each by host clock around decode_batch() (which ends in a synchronise), the median window: us per step.
The worker API times no batched attention launch on its own, so the attention is measured as a difference of whole steps: everything
but the attention launch is the same at every context, hence (us per step at n keys - us per step at 1 key) / layers = what the n keys
add to one attention launch.  The same figure of the 128-wide batched kernel (an 18-layer model with 8 heads over 1 kv head of 128,
fused at every level: the same grid) at TWICE the keys -- the same bytes of cache read per head -- stands next to it.  The cache holds whatever
the allocation left: the time does not depend on the values."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth


def _arg(name, default):
    return [int(a) for a in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default


L = ia.lib()
ROWS, KEYS = _arg("--rows", [2, 8, 16, 32]), _arg("--keys", [32, 512, 2048])
WINDOWS, WINDOW_S, MAX_CALLS = 3, 0.3, 200
GEMMA_2B = dict(layers=18, dim=2048, heads=8, kv_heads=1, head_dim=256, ffn=16384, vocab=32000)
WIDE128 = dict(layers=18, dim=1024, heads=8, kv_heads=1, head_dim=128, ffn=4096, vocab=32000)


def window(wk, n, keys, calls):
    toks, pos, slots = [7 + r for r in range(n)], [keys - 1] * n, list(range(n))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        wk.decode_batch(toks, pos, slots)
    return (time.perf_counter() - t0) / calls * 1e6


def median_us(wk, n, keys, levels):
    """{level: (median us per step, the windows)}: the levels alternate window by window"""
    calls, us = {}, {lv: [] for lv in levels}
    for lv in levels:                       # warm-up (the captured step of this row count), and the calls of a window from one call
        L.ifa_attention_mfma_heads(lv)
        window(wk, n, keys, 1)
        calls[lv] = max(1, min(MAX_CALLS, int(WINDOW_S * 1e6 / window(wk, n, keys, 1))))
    for _ in range(WINDOWS):
        for lv in levels:
            L.ifa_attention_mfma_heads(lv)
            us[lv].append(window(wk, n, keys, calls[lv]))
    return {lv: (sorted(us[lv])[WINDOWS // 2], us[lv]) for lv in levels}


def main():
    print("cache rows  keys | level 0 us | level 2 us | ratio | attn256 +us | 128-wide at 2 x keys +us   (windows level 0 / level 2)", flush=True)
    for kvd, name in ((dt.F16, "F16"), (dt.Q8_B32T2, "Q8")):
        wk, _, _ = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=max(KEYS) + 64, quant_threshold=0, **GEMMA_2B)
        ref, _, _ = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=2 * max(KEYS) + 64, quant_threshold=0, **WIDE128)
        wk.kv_slots(max(ROWS))
        ref.kv_slots(max(ROWS))
        L.ifa_attention_mfma_heads(2)
        assert L.ifa_model_batch_steps_rows(wk._h) == 32 and L.ifa_model_batch_steps_rows(ref._h) == 32
        for n in ROWS:
            base = median_us(wk, n, 1, (2,))[2][0]
            base128 = median_us(ref, n, 1, (2,))[2][0]
            for keys in KEYS:
                m = median_us(wk, n, keys, (0, 2))
                m128 = median_us(ref, n, 2 * keys, (2,))[2][0]
                print("%5s %4d %5d | %10.1f | %10.1f | %5.2f | %11.1f | %8.1f   (%s / %s)" % (
                    name, n, keys, m[0][0], m[2][0], m[0][0] / m[2][0], (m[2][0] - base) / GEMMA_2B["layers"], (m128 - base128) / WIDE128["layers"],
                    " ".join("%.0f" % t for t in m[0][1]), " ".join("%.0f" % t for t in m[2][1])), flush=True)
        L.ifa_attention_mfma_heads(0)
        wk.close()
        ref.close()


if __name__ == "__main__":
    main()
