"""-m gpu: the prompt routes agree with the routes they replace (same rows, other kernels: agreement within the F16 rounding of the
summation order), on two layers of Llama-2-7B width, and every run asserts the route it took (Worker.prompt_route, DESIGN.md "Prompt
route plan"):
  * 34..48 tokens: two passes of the rows GEMM (32 + the rest; option prefill_chunk, with prefill_mid 0 -- since round 6 k_gemm_mid takes
    these lengths in one pass) against the single pass;
  * 48..128 tokens: the four large-tile launches per layer (option prefill_big_min 47, with four parts of K for products of 32..96
    tiles; prefill_mid 0 likewise) against the op-by-op layer (prefill_big_min 128);
  * the edges of prefill_mid_max / prefill_res_mid, lowered to 64 / 96 tokens, against the op-by-op layer."""
import numpy as np
import pytest
import torch

from inferflow_amd import dtypes as dt, synth
from tests import gpu_util as g

pytestmark = pytest.mark.gpu


def _rows(wk, toks, V):
    lg = torch.empty((len(toks), V), dtype=torch.float16, device="cuda")
    wk.reset()
    tok = wk.forward(toks, 0, lg)
    return int(tok), g.host(lg).astype(np.float32)


def _agree(a, b):
    cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
    return cos >= 0.9999 and float(np.abs(a - b).max()) <= 0.02 * float(b.std()) + 0.01, (cos, float(np.abs(a - b).max()), float(b.std()))


def _route(wk):
    """(kind, first_pass, res_mid) of the last prompt"""
    r = wk.prompt_route()
    return r["kind"], r["first_pass"], r["res_mid"]


def _single_pass(T):
    """the one-pass route of T tokens with prefill_mid 0 at the default prefill_big_min (47)"""
    return ("big" if T > 47 else "op_by_op", 0, 0)


@pytest.mark.parametrize("T", [34, 40, 48])
def test_two_pass_prompt_agrees_with_the_single_pass(T):
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, dt.F16, max_ctx=64, layers=2, vocab=2000)
    toks = np.random.default_rng(T).integers(3, s["vocab"], T).astype(np.int32)
    wk.set_option("prefill_mid", 0)                 # (with it these lengths are ONE pass of k_gemm_mid whatever prefill_chunk says)
    out = {}
    for v in (1, 0):
        wk.set_option("prefill_chunk", v)
        out[v] = _rows(wk, toks, s["vocab"])
        assert _route(wk) == (("rows", 32, 0) if v else _single_pass(T))
    ok, why = _agree(out[1][1], out[0][1])          # ALL rows: the first pass's logits land in rows 0..31, the second's behind them
    assert ok, why
    wk.close()


@pytest.mark.parametrize("T", [48, 64, 128])
def test_short_prompt_large_tile_route_agrees_with_the_op_by_op_layer(T):
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, dt.F16, max_ctx=160, layers=2, vocab=2000)
    toks = np.random.default_rng(T).integers(3, s["vocab"], T).astype(np.int32)
    out = {}
    wk.set_option("prefill_chunk", 0)
    wk.set_option("prefill_mid", 0)                 # (with it both runs are k_gemm_mid's)
    for v in (47, 128):
        wk.set_option("prefill_big_min", v)
        out[v] = _rows(wk, toks, s["vocab"])
        assert _route(wk) == (("big", 0, 0) if v == 47 else ("op_by_op", 0, 0))
    ok, why = _agree(out[47][1], out[128][1])
    assert ok, why
    wk.close()


@pytest.mark.parametrize("T", [40, 64, 128])
def test_short_prompt_routes_match_the_oracle(T):
    """... and against the ORACLE (the reference's T > 1 rule: F16 activations x dequantised weights, fp32 sums), not only against each
    other: two layers of Llama-2-7B width, the model read back from the worker, every row of the prompt.  At the default options all
    three lengths are one pass of k_gemm_mid; with prefill_mid 0, 40 tokens = two passes of the rows GEMM, 64 / 128 = the large-tile
    launches with four parts of K.  Measured (r05): worst row 0.006-0.007 x std(logits) at 2 layers; bound 0.03 x std
    on every row (the whole-model law of test_gpu_fullsize_oracle would allow 0.08 sqrt(2) = 0.11), cosine >= 0.9999."""
    from tests import model_util as mu
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, dt.F16, max_ctx=160, layers=2, vocab=2000)
    om = mu.oracle_model_from_worker(wk, s, 160)
    toks = np.random.default_rng(100 + T).integers(3, s["vocab"], T).astype(np.int32)
    t_or, l_or = om.forward(toks, 0, nthreads=8)
    ref = l_or.astype(np.float32)
    std = float(ref.std())
    for mid, want in ((1, ("mid", 0, 0)), (0, ("rows", 32, 0) if T == 40 else ("big", 0, 0))):
        wk.set_option("prefill_mid", mid)
        tok, rows = _rows(wk, toks, s["vocab"])
        assert _route(wk) == want
        worst = 0.0
        for i in range(T):
            cos = float((rows[i] * ref[i]).sum() / (np.linalg.norm(rows[i]) * np.linalg.norm(ref[i])))
            mad = float(np.abs(rows[i] - ref[i]).max())
            worst = max(worst, mad / std)
            assert cos >= 0.9999 and mad <= 0.03 * std, (mid, i, cos, mad / std)
        top2 = np.sort(ref[-1])[-2:]
        if top2[1] - top2[0] > 0.03 * std:
            assert tok == int(t_or)
        print("T=%d prefill_mid %d worst row %.4f x std" % (T, mid, worst))
    wk.close()


def test_mid_route_edges_agree_with_the_op_by_op_layer():
    """The edges of the k_gemm_mid routes with the options lowered instead of the prompt raised: prefill_mid_max 64 (33 and 64 tokens: all
    four products through k_gemm_mid; 65: the large tiles), prefill_res_mid 96 (65 and 96 tokens: wo / w2 still through k_gemm_mid; 97:
    no more).  Each against the op-by-op layer of the same prompt."""
    wk, _, s = synth.build("llama2_7b", dt.Q4_B32T1A, dt.F16, max_ctx=160, layers=2, vocab=2000)
    routed = dict(prefill_mid=1, prefill_big=1, prefill_mid_max=64, prefill_res_mid=96)
    plain = dict(prefill_mid=0, prefill_big=0, prefill_chunk=0)
    want = {33: ("mid", 0, 0), 64: ("mid", 0, 0), 65: ("big", 0, 1), 96: ("big", 0, 1), 97: ("big", 0, 0)}
    for T in (33, 64, 65, 96, 97):
        toks = np.random.default_rng(200 + T).integers(3, s["vocab"], T).astype(np.int32)
        for k, v in routed.items():
            wk.set_option(k, v)
        _, got = _rows(wk, toks, s["vocab"])
        assert _route(wk) == want[T], T
        for k, v in plain.items():
            wk.set_option(k, v)
        _, ref = _rows(wk, toks, s["vocab"])
        assert _route(wk) == ("op_by_op", 0, 0), T
        wk.set_option("prefill_chunk", 1)
        ok, why = _agree(got, ref)
        assert ok, (T, why)
    wk.close()
