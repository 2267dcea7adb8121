"""-m gpu: the decode worker (op-by-op forward and the fused/graph decode)
against the whole-model oracle on small synthetic models."""
import numpy as np
import pytest
import torch

import oracle as o
from inferflow_amd import dtypes as dt, synth
from tests import gpu_util as g
from tests.model_util import oracle_model_from_host

pytestmark = pytest.mark.gpu
LOGIT_TOL = 0.03      # stated bound on |dlogit| vs the oracle (logit std ~0.5); greedy ids are compared whenever the oracle's top-2 gap exceeds it

CASES = [
    ("test_gqa", dt.Q4_B32T1A, dt.F16),
    ("test_mha", dt.Q4_B32T1A, dt.Q8_B32T2),
    ("test_gqa", dt.Q4_B32T1B, dt.Q8_B32T2),
    # the other int8-GEMV weight formats through the same fused kernels (C3 = Q3H + Q8 KV)
    ("test_gqa", dt.Q3H_B64T1, dt.Q8_B32T2),
    ("test_mha", dt.Q8_B32T2, dt.F16),
    ("test_gqa", dt.Q4_B64T1, dt.F16),
    ("test_mha", dt.Q5_B64T1, dt.Q8_B32T2),
    ("test_gqa", dt.Q6_B64T1, dt.F16),
    # fp16-activation tensors in the same 5-launch step (k_dec_gemv_h): whole F16 models (bin/llm_inference.tiny.ini is one,
    # 48-wide heads), the block formats outside the int8 path (gemv.h:632-1497), and layers the tensor_quant_threshold rule
    # leaves partly F16 (network_builder.cc:1557-1562: here wk / wv stay F16 next to a quantised wq)
    ("test_tiny", dt.F16, dt.F16),
    ("tiny15m", dt.F16, dt.F16),
    ("test_gqa", dt.F16, dt.Q8_B32T2),
    ("test_gqa", dt.Q8_B32T1, dt.F16),
    ("test_mha", dt.Q5_B32T1, dt.Q8_B32T2),
    ("test_gqa", dt.Q4_B16, dt.F16),
    ("test_gqa", dt.Q3_B32T1A, dt.F16),
    ("test_mha", dt.Q2_B32T1B, dt.F16),
    ("test_gqa", dt.Q4_B32T1A, dt.F16, 40000),
    ("test_gqa", dt.Q3H_B64T1, dt.Q8_B32T2, 100000),
]
CASE_IDS = ["gqa_q4_kvf16", "mha_q4_kvq8", "gqa_q4b_kvq8", "gqa_q3h_kvq8", "mha_q8_kvf16", "gqa_q4b64_kvf16",
            "mha_q5_kvq8", "gqa_q6_kvf16", "tiny_f16_hd48", "tiny15m_f16", "gqa_f16_kvq8", "gqa_q8t1", "mha_q5b32_kvq8",
            "gqa_q4b16", "gqa_q3", "mha_q2", "gqa_q4_kv_f16_by_threshold", "gqa_q3h_only_ffn_quantised"]
CASES = [c if len(c) == 4 else c + (0,) for c in CASES]


def _logits_close(a, b):
    a = a.astype(np.float32); b = b.astype(np.float32)
    cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
    return cos, float(np.abs(a - b).max())


@pytest.mark.parametrize("shape,wd,kvd,threshold", CASES, ids=CASE_IDS)
def test_forward_and_fused_decode_match_oracle(shape, wd, kvd, threshold):
    max_ctx = 64
    wk, host, s = synth.build(shape, wd, kvd, max_ctx=max_ctx, quant_threshold=threshold, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, kvd)
    ok, why = wk.fused_supported()
    assert ok, why
    rng = np.random.default_rng(42)
    prompt = rng.integers(3, s["vocab"], 9).astype(np.int32)

    # --- prefill (op-by-op, T>1) with full logits, like return_output_tensors
    lg = torch.empty((len(prompt), s["vocab"]), dtype=torch.float16, device="cuda")
    tok_gpu = wk.forward(prompt, 0, lg)
    tok_orc, lg_orc = om.forward(prompt, 0)
    cos, mad = _logits_close(g.host(lg), lg_orc)
    # fp tolerance: device expf/powf/sinf + attention summation order, amplified by
    # re-quantisation; stated bound: cosine >= 0.9995 and |dlogit| <= 0.03 (logit std ~0.5)
    assert cos >= 0.9995 and mad <= 0.03, (cos, mad)
    top2 = np.sort(lg_orc[-1].astype(np.float32))[-2:]
    if top2[1] - top2[0] > LOGIT_TOL:
        assert tok_gpu == tok_orc

    # --- fused + graph decode vs oracle, greedy, token by token: the ids must be the oracle's whenever the oracle's
    # top-2 gap exceeds the stated logit tolerance; steps inside it (a tie at this precision) follow the GPU and are counted
    n_steps = 12
    toks_fused, ms = wk.decode(tok_gpu, len(prompt), n_steps)
    assert ms > 0
    cur, excused = tok_gpu, 0
    for i in range(n_steps):
        t_or, l_or = om.forward(np.array([cur], np.int32), len(prompt) + i)
        top2 = np.sort(l_or[0].astype(np.float32))[-2:]
        if top2[1] - top2[0] <= LOGIT_TOL:
            excused += int(int(toks_fused[i]) != t_or)
            cur = int(toks_fused[i]); continue
        assert int(toks_fused[i]) == t_or, "step %d" % i
        cur = t_or
    assert excused <= 2, excused

    # --- fused decode == op-by-op decode on the same worker (same rounding points)
    wk.reset()
    wk.forward(prompt, 0)
    wk.set_option("fused", 0)
    toks_ops, _ = wk.decode(tok_gpu, len(prompt), n_steps)
    wk.set_option("fused", 1)
    assert np.array_equal(toks_ops, toks_fused)
    # --- and eager fused (no graph) == graph replay, bit for bit
    wk.reset()
    wk.forward(prompt, 0)
    wk.set_option("graph", 0)
    toks_eager, _ = wk.decode(tok_gpu, len(prompt), n_steps)
    lg_eager = wk.read_buffer("logits").copy()
    wk.set_option("graph", 1)
    wk.reset()
    wk.forward(prompt, 0)
    toks_graph, _ = wk.decode(tok_gpu, len(prompt), n_steps)
    assert np.array_equal(toks_eager, toks_graph)
    assert np.array_equal(lg_eager, wk.read_buffer("logits"))
    wk.close()


@pytest.mark.parametrize("wd,kvd", [(dt.Q4_B32T1A, dt.F16), (dt.Q3H_B64T1, dt.Q8_B32T2)], ids=["q4_kvf16", "q3h_kvq8"])
def test_long_prompt_prefill_matches_oracle_with_and_without_the_large_tile_kernel(wd, kvd):
    """A 150-token prompt: every linear layer through the in-tree prefill kernels (the large-tile kernel above 128 tokens, four
    launches per layer for the Q4 model; the smaller-tile kernels with prefill_big = 0), the attention the MFMA prefill kernel.
    Same tolerance against the oracle as the short-prompt case, and the two kernel families agree with each other."""
    max_ctx = 192
    wk, host, s = synth.build("test_gqa", wd, kvd, max_ctx=max_ctx, quant_threshold=0, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, kvd)
    prompt = np.random.default_rng(8).integers(3, s["vocab"], 150).astype(np.int32)
    lg = torch.empty((len(prompt), s["vocab"]), dtype=torch.float16, device="cuda")
    wk.set_option("prefill_big", 0)
    tok_small = wk.forward(prompt, 0, lg)
    lg_small = g.host(lg).copy()
    tok_orc, lg_orc = om.forward(prompt, 0, nthreads=4)
    cos, mad = _logits_close(lg_small, lg_orc)
    assert cos >= 0.9995 and mad <= 0.03, (cos, mad)
    wk.set_option("prefill_big", 1)
    wk.reset()
    tok_own = wk.forward(prompt, 0, lg)
    cos1, mad1 = _logits_close(g.host(lg), lg_orc)
    assert cos1 >= 0.9995 and mad1 <= 0.03, (cos1, mad1)
    cos2, mad2 = _logits_close(g.host(lg), lg_small)
    assert cos2 >= 0.9999 and mad2 <= 0.02, (cos2, mad2)
    top2 = np.sort(lg_orc[-1].astype(np.float32))[-2:]
    if top2[1] - top2[0] > LOGIT_TOL:
        assert tok_small == tok_orc == tok_own
    wk.close()


def test_kv_cache_rows_match_oracle_after_prefill():
    wk, host, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.Q8_B32T2, max_ctx=32, quant_threshold=0, std=0.06, keep_host=True)
    prompt = np.arange(5, 12, dtype=np.int32)
    wk.forward(prompt, 0)
    kv_dim = s["kv_heads"] * s["head_dim"]
    rb = dt.row_bytes(dt.Q8_B32T2, kv_dim)
    k0 = wk.read_buffer("kcache", 0, nbytes=rb * len(prompt)).reshape(len(prompt), rb)
    # layer-0 K rows depend only on embeddings, norm, wk GEMV (fp16-activation path), RoPE, Q8 quantiser
    om = oracle_model_from_host(host, s, 32, dt.Q8_B32T2)
    om.forward(prompt, 0)
    deq_gpu = o.dequantize(dt.Q8_B32T2, k0, kv_dim).astype(np.float32)
    # oracle cache is private; recompute layer-0 K through the op-level oracle instead
    emb = host[(-1, 0)][1].reshape(s["vocab"], s["dim"])[prompt]
    xn = o.rmsnorm(emb, host[(0, 10)][1].reshape(-1))
    wkq = o.quantize(dt.Q4_B32T1A, host[(0, 13)][1].reshape(kv_dim, s["dim"]))
    k = np.stack([o.gemv_f16x(dt.Q4_B32T1A, wkq, kv_dim, s["dim"], xn[t]) for t in range(len(prompt))])
    k = o.rope(k.reshape(len(prompt), s["kv_heads"], s["head_dim"]), 0).reshape(len(prompt), kv_dim)
    deq_orc = o.dequantize(dt.Q8_B32T2, o.quantize_act_q8(k), kv_dim).astype(np.float32)
    assert np.abs(deq_gpu - deq_orc).max() <= 0.02 * np.abs(deq_orc).max()
    wk.close()


def test_decode_rejects_out_of_range_positions():
    wk, _, s = synth.build("test_gqa", max_ctx=16, quant_threshold=0)
    rc = g.capi().ifa_model_decode(wk._h, 1, 10, 10, None, None)
    assert rc == -1 and b"max_ctx" in g.capi().ifa_last_error()
    rc = g.capi().ifa_model_forward(wk._h, None, 1, 0, None, None)
    assert rc == -1
    wk.close()


FALCON_LIKE = dict(norm_kind=1, act_kind=1, is_glu=0, parallel_attn=1, rope_order=1)


def _build_custom(shape, wd, kvd, max_ctx, cfg, with_bias=False, std=0.06, post=None):
    """A worker + oracle pair for non-llama wiring (std norm, GELU, no w3, parallel attention, biases)."""
    import oracle as o
    from inferflow_amd import worker as W
    s = dict(synth.SHAPES[shape])
    wk = W.DecodeWorker(max_ctx=max_ctx, kv_dtype=kvd, **s, **cfg)
    om = o.Model(max_ctx=max_ctx, kv_dtype=kvd, **s, **cfg)
    rng = np.random.default_rng(11)

    def put(layer, tid, target, arr):
        arr16 = arr.astype(np.float16)
        rows, cols = (1, arr16.size) if arr16.ndim == 1 else arr16.shape
        wk.set_tensor_f16(layer, tid, target, g.dev(arr16), rows, cols)
        data = arr16.reshape(rows, cols).view(np.uint16) if target == dt.F16 else o.quantize(target, arr16.reshape(rows, cols))
        om.set_tensor(max(layer, 0), tid, target, data, rows, cols)

    d, qd, kvdim, f, v = s["dim"], s["heads"] * s["head_dim"], s["kv_heads"] * s["head_dim"], s["ffn"], s["vocab"]
    put(-1, W.T_EMBD, dt.F16, rng.normal(0, std, (v, d)))
    put(-1, W.T_OUT_NORM, dt.F16, rng.normal(1, 0.1, d)); put(-1, W.T_OUT_NORM_B, dt.F16, rng.normal(0, 0.05, d))
    put(-1, W.T_LM_HEAD, dt.F16, rng.normal(0, std, (v, d)))
    for l in range(s["layers"]):
        if post != "only":
            put(l, W.T_ATTN_NORM, dt.F16, rng.normal(1, 0.1, d)); put(l, W.T_ATTN_NORM_B, dt.F16, rng.normal(0, 0.05, d))
        for tid, shp in [(W.T_WQ, (qd, d)), (W.T_WK, (kvdim, d)), (W.T_WV, (kvdim, d)), (W.T_WO, (d, qd)),
                         (W.T_W1, (f, d)), (W.T_W2, (d, f))]:
            put(l, tid, wd, rng.normal(0, std, shp))
        if cfg.get("is_glu", 1):
            put(l, W.T_W3, wd, rng.normal(0, std, (f, d)))
        if not cfg.get("parallel_attn") and post != "only":
            put(l, W.T_FFN_NORM, dt.F16, rng.normal(1, 0.1, d))
        if post:      # self_attn.post_norm / feed_forward.post_norm (+ biases)
            put(l, W.T_ATTN_POST_NORM, dt.F16, rng.normal(1, 0.1, d)); put(l, W.T_ATTN_POST_NORM_B, dt.F16, rng.normal(0, 0.05, d))
            put(l, W.T_FFN_POST_NORM, dt.F16, rng.normal(1, 0.1, d)); put(l, W.T_FFN_POST_NORM_B, dt.F16, rng.normal(0, 0.05, d))
        if with_bias:
            for tid, n in [(W.T_WQ_B, qd), (W.T_WK_B, kvdim), (W.T_WV_B, kvdim), (W.T_WO_B, d), (W.T_W1_B, f), (W.T_W2_B, d)]:
                put(l, tid, dt.F16, rng.normal(0, 0.05, n))
    wk.finalize()
    return wk, om, s


FALCON40_LIKE = dict(norm_kind=1, act_kind=1, is_glu=0, share_input=1, rope_order=2)      # two norms on the layer input
BLOOM_LIKE = dict(norm_kind=1, act_kind=1, is_glu=0, rope_order=0, use_alibi=1)             # sequential, std norm, ALiBi
RMS_PARALLEL = dict(parallel_attn=1)                                                       # llama-style weights, parallel wiring
# RMS weight = 1 + w, GELU-gated, embeddings * sqrt(dim) (has_embedding_linear_norm: LinearNorm, inference_worker.cc:447-451)
GEMMA_LIKE = dict(attn_norm_base=1.0, ffn_norm_base=1.0, out_norm_base=1.0, act_kind=1, embd_scale=-1.0)
# TensorOpr::Scale on the outputs + embedding_linear_scale 12 (data/models/minicpm_2b_dpo_bf16/model_spec.json)
MINICPM_LIKE = dict(attn_out_scale=0.25, ffn_out_scale=0.25, out_scale=0.111111, embd_scale=12.0)


@pytest.mark.parametrize("name,cfg,bias", [("falcon_like", FALCON_LIKE, True), ("falcon40_like", FALCON40_LIKE, False),
                                            ("bloom_like", BLOOM_LIKE, True), ("rms_parallel", RMS_PARALLEL, False),
                                            ("gemma_like", GEMMA_LIKE, False), ("minicpm_like", MINICPM_LIKE, False),
                                            ("minicpm_parallel", dict(MINICPM_LIKE, parallel_attn=1), True),
                                            ("llama_bias_q8kv", dict(), True)])
def test_other_wirings_fused_and_op_path(name, cfg, bias):
    """Std-norm / GELU / non-gated FFN / parallel attention / shared input / ALiBi / bias models: the op-by-op path
    against the oracle, and the fused decode (norm as its own launch for std-norm models, residuals folded into the
    W2 epilogue) bit for bit against the op-by-op decode."""
    kvd = dt.Q8_B32T2 if "q8kv" in name else dt.F16
    wk, om, s = _build_custom("test_gqa", dt.Q4_B32T1A, kvd, 32, cfg, with_bias=bias)
    ok, why = wk.fused_supported()
    assert ok, why          # output scales (MiniCPM) are folded into the Wo / W2 epilogues like the residuals
    prompt = np.array([7, 99, 512, 3, 41], np.int32)
    lg = torch.empty((len(prompt), s["vocab"]), dtype=torch.float16, device="cuda")
    tok = wk.forward(prompt, 0, lg)
    tok_o, lg_o = om.forward(prompt, 0, nthreads=4)
    cos, mad = _logits_close(g.host(lg), lg_o)
    assert cos >= 0.9995 and mad <= 0.02 * float(np.abs(lg_o.astype(np.float32)).max()) + 0.02, (cos, mad)
    toks, _ = wk.decode(tok, len(prompt), 6)
    lg_fused = wk.read_buffer("logits").copy()
    cur = tok
    for i in range(6):
        t_o, l_o = om.forward(np.array([cur], np.int32), len(prompt) + i, nthreads=4)
        top2 = np.sort(l_o[0].astype(np.float32))[-2:]
        assert int(toks[i]) == t_o or top2[1] - top2[0] <= LOGIT_TOL, "step %d" % i
        cur = int(toks[i])
    wk.set_option("fused", 0)
    toks_ops, _ = wk.decode(tok, len(prompt), 6)
    assert np.array_equal(toks, toks_ops)
    assert np.array_equal(lg_fused, wk.read_buffer("logits"))
    wk.close()


@pytest.mark.parametrize("name,cfg,post,as_res", [
    ("post_ln_only", dict(norm_kind=1, act_kind=2, is_glu=0), "only", 1),          # BERT / OPT-350m style: no pre norms, both post norms
    ("pre_and_post", dict(), "both", 1),                                           # pre norms + post norms, the residual follows the post norm
    ("pre_and_post_residual_before", dict(), "both", 0),                           # is_attn_post_as_residual = false (Mixtral's spec form)
    ("post_parallel", dict(norm_kind=1, act_kind=1, is_glu=0, parallel_attn=1), "both", 1)])
def test_post_norm_wirings_match_oracle(name, cfg, post, as_res):
    """self_attn.post_norm / feed_forward.post_norm and is_attn_post_as_residual (ProcessGpuLayer, inference_worker.cc:857-866,
    954-965; model.h:113): the op-by-op layer against the oracle on a prompt and on single-token steps (such models decline the
    fused launches: decode runs the same ops token by token), and the batched step against the single-query steps."""
    wk, om, s = _build_custom("test_gqa", dt.Q4_B32T1A, dt.F16, 32, cfg, with_bias=True, post=post)
    wk.set_option("attn_post_as_residual", as_res)
    om.set_attn_post_as_residual(as_res)
    ok, why = wk.fused_supported()
    assert not ok and "post norm" in why
    prompt = np.array([7, 99, 512, 3, 41], np.int32)
    lg = torch.empty((len(prompt), s["vocab"]), dtype=torch.float16, device="cuda")
    tok = wk.forward(prompt, 0, lg)
    tok_o, lg_o = om.forward(prompt, 0, nthreads=4)
    cos, mad = _logits_close(g.host(lg), lg_o)
    assert cos >= 0.9995 and mad <= 0.02 * float(np.abs(lg_o.astype(np.float32)).max()) + 0.02, (name, cos, mad)
    toks, _ = wk.decode(tok, len(prompt), 5)
    cur = tok
    for i in range(5):
        t_o, l_o = om.forward(np.array([cur], np.int32), len(prompt) + i, nthreads=4)
        top2 = np.sort(l_o[0].astype(np.float32))[-2:]
        assert int(toks[i]) == t_o or top2[1] - top2[0] <= LOGIT_TOL, "step %d" % i
        cur = int(toks[i])
    # the flag matters: the other setting gives different logits on the same weights
    om.reset(); om.set_attn_post_as_residual(1 - as_res)
    _, lg_other = om.forward(prompt, 0, nthreads=4)
    assert np.abs(lg_other.astype(np.float32) - lg_o.astype(np.float32)).max() > 0.05
    wk.close()


@pytest.mark.parametrize("wd,kvd", [(dt.Q4_B32T1A, dt.F16), (dt.Q3H_B64T1, dt.Q8_B32T2)], ids=["q4", "q3h_kvq8"])
def test_moe_layers_match_oracle(wd, kvd):
    """Mixtral-style mixture of experts (ProcessGpuLayer_Moe): router GEMV, softmax, top-2 with renormalisation,
    expert FFNs in ascending order, half-precision scatter-add -- op path (host routing, like the reference) and
    fused decode (device routing, expert weights through a pointer table) against the oracle and each other."""
    max_ctx = 48
    wk, host, s = synth.build("test_moe", wd, kvd, max_ctx=max_ctx, quant_threshold=0, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, kvd)
    ok, why = wk.fused_supported()
    assert ok, why
    prompt = np.random.default_rng(5).integers(3, s["vocab"], 6).astype(np.int32)
    lg = torch.empty((len(prompt), s["vocab"]), dtype=torch.float16, device="cuda")
    tok = wk.forward(prompt, 0, lg)
    tok_o, lg_o = om.forward(prompt, 0, nthreads=4)
    cos, mad = _logits_close(g.host(lg), lg_o)
    assert cos >= 0.9995 and mad <= 0.03, (cos, mad)
    n = 10
    assert wk.moe_plan(0, 1)["router"] == "fused"      # (which router the step runs: the plan the engine follows, not the option alone)
    fused, _ = wk.decode(tok, len(prompt), n)
    logits_fused = wk.read_buffer("logits").copy()
    cur = tok
    for i in range(n):
        t_or, l_or = om.forward(np.array([cur], np.int32), len(prompt) + i, nthreads=4)
        top2 = np.sort(l_or[0].astype(np.float32))[-2:]
        if top2[1] - top2[0] > LOGIT_TOL:
            assert int(fused[i]) == t_or, "step %d" % i
        cur = int(fused[i])
    wk.set_option("fused", 0)
    unfused, _ = wk.decode(tok, len(prompt), n)        # op-by-op steps with the reference's host-side routing
    assert np.array_equal(fused, unfused)
    assert np.array_equal(logits_fused, wk.read_buffer("logits"))
    # the router as four launches (norm, gate GEMV, softmax, k_moe_topk) instead of the one-launch k_dec_moe_router: same bits
    wk.set_option("fused", 1); wk.set_option("moe_router_fused", 0)
    assert wk.moe_plan(0, 1)["router"] == "ops"
    wk.reset(); wk.forward(prompt, 0)
    four, _ = wk.decode(tok, len(prompt), n)
    assert np.array_equal(fused, four)
    assert np.array_equal(logits_fused, wk.read_buffer("logits"))
    wk.close()


# rows -> (tile_rows, max_tiles, small_max) of the layer's plan (4 experts, top 2: tests/test_moe_plan_cpu.py has the table and the rules)
MOE_PREFILL_PLANS = {2: (64, 0, 8), 8: (64, 0, 8), 9: (64, 4, 8), 16: (64, 4, 8), 17: (64, 4, 0), 37: (64, 5, 0), 128: (64, 8, 0), 192: (128, 7, 0),
                     300: (128, 8, 0)}


@pytest.mark.parametrize("T", sorted(MOE_PREFILL_PLANS))
def test_moe_prefill_device_routed_grouped_path(T):
    """MoE over T > 1 rows without the host: device routing, device-built per-expert row lists, ONE grouped MFMA launch
    per product over the experts with >= 2 rows and one grouped int8-GEMV launch over the single-row experts
    (moe_ffn_device) -- against the oracle (which restates the reference's host-routed expert loop, incl. its T = 1
    branch for single-row experts) and against the host-routed op path of this library.  The row counts are those at which
    the layer's plan changes (small groups / tiles / tile height); the plan the engine follows says which route each run took."""
    max_ctx = 320
    wk, host, s = synth.build("test_moe", dt.Q4_B32T1A, dt.F16, max_ctx=max_ctx, quant_threshold=0, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, dt.F16)
    prompt = np.random.default_rng(100 + T).integers(3, s["vocab"], T).astype(np.int32)
    lg = torch.empty((T, s["vocab"]), dtype=torch.float16, device="cuda")
    wk.set_option("moe_device", 1)
    for layer in range(s["layers"]):
        p = wk.moe_plan(layer, T)
        assert p["kind"] in ("device_grouped", "device_singles") and p["host_sync"] == 0 and p["cap"] == 2 * T, p
        assert (p["tile_rows"], p["max_tiles"], p["small_max"]) == MOE_PREFILL_PLANS[T], p
    tok_dev = wk.forward(prompt, 0, lg)
    lg_dev = g.host(lg).copy()
    wk.set_option("moe_device", 0)
    p = wk.moe_plan(0, T)
    assert p["kind"] == "host" and p["host_sync"] == 1 and p["device_ok"] == 0, p
    tok_host = wk.forward(prompt, 0, lg)
    lg_host = g.host(lg).copy()
    cos, mad = _logits_close(lg_dev, lg_host)
    assert cos >= 0.99995 and mad <= 0.02, (cos, mad)          # same arithmetic; the per-expert products go through kernels of different shape (2-8 rows: the weight-streaming rows kernel; split-K widths)
    if T <= 128:                                                # (the oracle's scalar loops take seconds per 100 tokens)
        tok_o, lg_o = om.forward(prompt, 0, nthreads=8)
        cos, mad = _logits_close(lg_dev, lg_o)
        assert cos >= 0.9995 and mad <= LOGIT_TOL, (cos, mad)
        top2 = np.sort(lg_o[-1].astype(np.float32))[-2:]
        if top2[1] - top2[0] > LOGIT_TOL:
            assert tok_dev == tok_o == tok_host
    wk.close()


@pytest.mark.parametrize("kvd", [dt.F16, dt.Q8_B32T2], ids=["kvf16", "kvq8"])
def test_long_context_split_attention_matches_single_workgroup_kernel(kvd):
    """Past `attn_split_ctx` the decode step spreads a head's keys over 8 workgroups (scores / P.V / combine): same
    rounding points as the one-workgroup kernel, only the order of the P.V partial sums changes."""
    wk, host, s = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=700, quant_threshold=0, std=0.06, keep_host=True)
    rng = np.random.default_rng(17)
    prompt = rng.integers(3, s["vocab"], 600).astype(np.int32)
    tok = wk.forward(prompt, 0)
    wk.set_option("attn_split_ctx", 0)            # never split
    ref, _ = wk.decode(tok, len(prompt), 24)
    lg_ref = wk.read_buffer("logits").view(np.float16).astype(np.float32)
    wk.set_option("attn_split_ctx", 64)           # split from the first step on
    got, _ = wk.decode(tok, len(prompt), 24)
    lg = wk.read_buffer("logits").view(np.float16).astype(np.float32)
    cos = float((lg * lg_ref).sum() / (np.linalg.norm(lg) * np.linalg.norm(lg_ref)))
    assert cos >= 0.9999 and np.abs(lg - lg_ref).max() <= 0.02, (cos, np.abs(lg - lg_ref).max())
    agree = np.mean(np.asarray(got) == np.asarray(ref))
    assert agree >= 0.9, (got, ref)               # greedy tokens may differ only at near ties
    # and against the oracle at this context
    om = oracle_model_from_host(host, s, 700, kvd)
    om.forward(prompt, 0, nthreads=8)
    t_or, l_or = om.forward(np.array([tok], np.int32), len(prompt), nthreads=8)
    top2 = np.sort(l_or[0].astype(np.float32))[-2:]
    if top2[1] - top2[0] > LOGIT_TOL:
        assert int(got[0]) == t_or
    wk.close()


@pytest.mark.parametrize("kvd", [dt.F16, dt.Q8_B32T2], ids=["kvf16", "kvq8"])
def test_dynamic_batching_rows_are_independent_queries(kvd):
    """ifa_model_decode_batch: one new token for each of n queries, every query on its own KV cache slot.  Rows must
    not interact (permutation / duplication give identical bits) and each row must agree with the same query decoded
    alone (alone = int8-activation GEMV path, batched = F16-activation MFMA GEMM path, like the reference's two
    MatrixMultiplication branches: compared within tolerance)."""
    wk, host, s = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=64, quant_threshold=0, std=0.06, keep_host=True)
    V = s["vocab"]
    wk.kv_slots(6)
    rng = np.random.default_rng(23)
    prompts = [rng.integers(3, V, n).astype(np.int32) for n in (5, 11, 8)]
    # one ORACLE per query (own KV cache), with the arithmetic of the reference's T > 1 branch that a batched step runs
    # (F16 activations on dequantised weights: MatrixMultiplication, inference_worker.cc:2374-2415)
    oms = [oracle_model_from_host(host, s, 64, kvd, full_quant_gemv=0) for _ in prompts]
    first = []
    for i, pr in enumerate(prompts):          # slots 0..2 (batched) and 3..5 (each query alone) hold the same prefills
        wk.select_kv(i); first.append(wk.forward(pr, 0))
        wk.select_kv(3 + i); assert wk.forward(pr, 0) == first[i]
        oms[i].forward(pr, 0, want_logits=False, nthreads=4)
    cur = list(first)
    pos = [len(p) for p in prompts]
    lg = torch.empty((3, V), dtype=torch.float16, device="cuda")
    lg1 = torch.empty((1, V), dtype=torch.float16, device="cuda")
    lgp = torch.empty((3, V), dtype=torch.float16, device="cuda")
    agree = total = 0
    for step in range(6):
        nxt = wk.decode_batch(cur, pos, [0, 1, 2], lg)
        rows = g.host(lg).copy()
        for i in range(3):                     # every batched row against the oracle of its query, engine-test tolerance
            t_o, l_o = oms[i].forward(np.array([cur[i]], np.int32), pos[i], nthreads=4)
            cos_o, mad_o = _logits_close(rows[i], l_o[0])
            assert cos_o >= 0.9995 and mad_o <= LOGIT_TOL, (step, i, cos_o, mad_o)
            top2 = np.sort(l_o[0].astype(np.float32))[-2:]
            if top2[1] - top2[0] > LOGIT_TOL:
                assert int(nxt[i]) == t_o, (step, i)
        for i in range(3):                     # the same step for query i alone, on its own copy of the cache
            wk.select_kv(3 + i)
            t1 = wk.forward(np.array([cur[i]], np.int32), pos[i], lg1)
            cos, mad = _logits_close(rows[i], g.host(lg1)[0])
            # Q8-quantised activations (alone) vs F16 activations (batched): ~1 % of the logit range
            assert cos >= 0.999 and mad <= 0.03 * float(np.abs(rows[i].astype(np.float32)).max()) + 0.03, (step, i, cos, mad)
            total += 1; agree += int(t1 == nxt[i])
            # feed the batched token to both copies so the two histories stay identical
        cur = [int(t) for t in nxt]
        pos = [p + 1 for p in pos]
    assert agree >= total - 3
    # permutation: the same step again with the rows in another order (a step only rewrites its own KV rows with the
    # same values, so repeating it is idempotent)
    a = wk.decode_batch(cur, pos, [0, 1, 2], lg)
    b = wk.decode_batch([cur[2], cur[0], cur[1]], [pos[2], pos[0], pos[1]], [2, 0, 1], lgp)
    assert [int(b[1]), int(b[2]), int(b[0])] == [int(t) for t in a]
    A, B = g.host(lg), g.host(lgp)
    assert np.array_equal(A[0], B[1]) and np.array_equal(A[1], B[2]) and np.array_equal(A[2], B[0])
    wk.close()


@pytest.mark.parametrize("kvd", [dt.F16, dt.Q8_B32T2], ids=["kvf16", "kvq8"])
def test_batched_step_at_contexts_past_the_prefetched_bucket(kvd):
    """Queries with several hundred cached keys in one batched step: k_dec_attn<.., BATCH> walks the keys past its 256-row entry prefetch
    in 256-key iterations (K rows one iteration ahead) and the V rows in double-buffered batches of eight keys (round 6).  Every row
    against the same query decoded alone on a copy of its cache through the single-query step (at these contexts: the keys-split-over-
    workgroups kernels; Q8 activations alone vs F16 activations batched: the tolerance of test_dynamic_batching_rows_are_independent_queries),
    the fused step against the op-by-op rows, and row order must not matter (identical bits under permutation)."""
    wk, host, s = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=720, quant_threshold=0, std=0.06, keep_host=True)
    V = s["vocab"]
    wk.kv_slots(6)
    rng = np.random.default_rng(29)
    prompts = [rng.integers(3, V, n).astype(np.int32) for n in (300, 517, 690)]
    first = []
    for i, pr in enumerate(prompts):
        wk.select_kv(i); first.append(wk.forward(pr, 0))
        wk.select_kv(3 + i); assert wk.forward(pr, 0) == first[i]
    cur, pos = list(first), [len(p) for p in prompts]
    lg = torch.empty((3, V), dtype=torch.float16, device="cuda")
    lgu = torch.empty((3, V), dtype=torch.float16, device="cuda")
    lg1 = torch.empty((1, V), dtype=torch.float16, device="cuda")
    agree = total = 0
    for step in range(5):
        wk.set_option("batch_fused", 1)
        nxt = wk.decode_batch(cur, pos, [0, 1, 2], lg)
        rows = g.host(lg).copy()
        for i in range(3):
            wk.select_kv(3 + i)
            t1 = wk.forward(np.array([cur[i]], np.int32), pos[i], lg1)
            cos, mad = _logits_close(rows[i], g.host(lg1)[0])
            assert cos >= 0.999 and mad <= 0.03 * float(np.abs(rows[i].astype(np.float32)).max()) + 0.03, (step, i, cos, mad)
            total += 1; agree += int(t1 == nxt[i])
        cur = [int(t) for t in nxt]
        pos = [p + 1 for p in pos]
    assert agree >= total - 3
    a = wk.decode_batch(cur, pos, [0, 1, 2], lg)
    wk.set_option("batch_fused", 0)
    wk.decode_batch(cur, pos, [0, 1, 2], lgu)                                  # op-by-op rows: same GEMM arithmetic, another attention kernel
    A, U = g.host(lg).astype(np.float32), g.host(lgu).astype(np.float32)
    cos = float((A * U).sum() / (np.linalg.norm(A) * np.linalg.norm(U)))
    assert cos >= 0.9999 and np.abs(A - U).max() <= 0.02, (cos, np.abs(A - U).max())
    wk.set_option("batch_fused", 1)
    lgp = torch.empty((3, V), dtype=torch.float16, device="cuda")
    b = wk.decode_batch([cur[2], cur[0], cur[1]], [pos[2], pos[0], pos[1]], [2, 0, 1], lgp)
    assert [int(b[1]), int(b[2]), int(b[0])] == [int(t) for t in a]
    A16, B16 = g.host(lg), g.host(lgp)
    wk.decode_batch(cur, pos, [0, 1, 2], lg)
    A16 = g.host(lg)
    assert np.array_equal(A16[0], B16[1]) and np.array_equal(A16[1], B16[2]) and np.array_equal(A16[2], B16[0])
    wk.close()


@pytest.mark.parametrize("n", [2, 5, 8, 11, 16, 20, 27, 32])
@pytest.mark.parametrize("kvd,shape", [(dt.F16, "test_mha"), (dt.Q8_B32T2, "test_mha"), (dt.F16, "test_moe"), (dt.F16, "test_moe_longffn")],
                         ids=["kvf16", "kvq8", "moe", "moe_longffn"])
def test_fused_batched_step_matches_op_by_op_rows_and_graph_replay(kvd, shape, n):
    """The batched decode step as five launches per layer (norm prologue + wq|wk|wv, batched k_dec_attn, wo + residual,
    norm + w1/w3 + GLU, w2 + residual: ifa_gemm_rows_mfma.hip, batch_fused_layer) against the op-by-op rows of the same
    library (same GEMM arithmetic; the attention kernels differ in summation order) and against its own graph replay.
    MoE layers: the attention half fused, the expert FFNs device-routed over the rows, the whole step still one graph."""
    wk, host, s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=48, quant_threshold=0, std=0.06, keep_host=True)
    V = s["vocab"]
    wk.kv_slots(2 * n)
    rng = np.random.default_rng(5 + n)
    prompts = [rng.integers(3, V, 3 + (i * 5) % 11).astype(np.int32) for i in range(n)]
    cur, pos = [], []
    for i, pr in enumerate(prompts):
        wk.select_kv(i); t = wk.forward(pr, 0)
        wk.select_kv(n + i); assert wk.forward(pr, 0) == t
        cur.append(t); pos.append(len(pr))
    lgf = torch.empty((n, V), dtype=torch.float16, device="cuda")
    lgu = torch.empty((n, V), dtype=torch.float16, device="cuda")
    for step in range(4):
        wk.set_option("batch_fused", 1)
        tf = wk.decode_batch(cur, pos, list(range(n)), lgf)                 # eager (logits requested)
        wk.set_option("batch_fused", 0)
        tu = wk.decode_batch(cur, pos, list(range(n, 2 * n)), lgu)          # op-by-op rows on the copies of the caches
        a, b = g.host(lgf).astype(np.float32), g.host(lgu).astype(np.float32)
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.9999 and np.abs(a - b).max() <= 0.02, (step, cos, np.abs(a - b).max())
        wk.set_option("batch_fused", 1)
        tg = wk.decode_batch(cur, pos, list(range(n)))                      # graph replay of the same step: idempotent on the caches
        assert [int(t) for t in tg] == [int(t) for t in tf], step
        gaps = np.sort(a, axis=1)
        for i in range(n):
            if gaps[i, -1] - gaps[i, -2] > LOGIT_TOL:
                assert int(tf[i]) == int(tu[i]), (step, i)
        cur = [int(t) for t in tf]
        pos = [p + 1 for p in pos]
    wk.close()


@pytest.mark.parametrize("n", [3, 8, 12, 20])
@pytest.mark.parametrize("wd", [dt.Q3H_B64T1, dt.Q4_B64T1], ids=["q3h", "q4_b64"])
def test_fused_batched_step_for_the_64_weight_nibble_formats(wd, n):
    """Q3H_B64T1 (as streamed: nibble pairs) and Q4_B64T1 have the value q * scale + base of Q4_B32T1 with one (base, scale) per
    64 weights: their MO copies write the word for both 32-weight halves and the fused batched step (rows GEMM on the matrix
    cores) runs unchanged.  Against the op-by-op rows of the same worker (generic GEMM on the reference-layout blocks: same
    dequantised halves, another summation order) and against its own graph replay; short prompts take the same kernels."""
    wk, _, s = synth.build("test_mha", wd, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)
    V = s["vocab"]
    wk.kv_slots(2 * n)
    rng = np.random.default_rng(70 + n)
    prompts = [rng.integers(3, V, 3 + (i * 5) % 11).astype(np.int32) for i in range(n)]
    cur, pos = [], []
    for i, pr in enumerate(prompts):
        wk.set_option("batch_fused", 1)
        wk.select_kv(i); lg1 = torch.empty((len(pr), V), dtype=torch.float16, device="cuda"); t = wk.forward(pr, 0, lg1)
        wk.set_option("batch_fused", 0)
        wk.select_kv(n + i); lg0 = torch.empty((len(pr), V), dtype=torch.float16, device="cuda"); wk.forward(pr, 0, lg0)
        a, b = g.host(lg1).astype(np.float32), g.host(lg0).astype(np.float32)
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.9999 and np.abs(a - b).max() <= 0.02, ("prompt", i, cos, np.abs(a - b).max())
        cur.append(t); pos.append(len(pr))
    lgf = torch.empty((n, V), dtype=torch.float16, device="cuda")
    lgu = torch.empty((n, V), dtype=torch.float16, device="cuda")
    for step in range(3):
        wk.set_option("batch_fused", 1)
        tf = wk.decode_batch(cur, pos, list(range(n)), lgf)
        wk.set_option("batch_fused", 0)
        wk.decode_batch(cur, pos, list(range(n, 2 * n)), lgu)
        a, b = g.host(lgf).astype(np.float32), g.host(lgu).astype(np.float32)
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.9999 and np.abs(a - b).max() <= 0.02, (step, cos, np.abs(a - b).max())
        wk.set_option("batch_fused", 1)
        tg = wk.decode_batch(cur, pos, list(range(n)))
        assert [int(t) for t in tg] == [int(t) for t in tf], step
        cur = [int(t) for t in tf]; pos = [p + 1 for p in pos]
    wk.close()


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 13, 16, 24])
@pytest.mark.parametrize("shape", ["test_mha", "test_gqa", "test_longffn"])
def test_rows_gemm_operand_order_copy_is_bit_identical_to_the_tiled_path(shape, n):
    """The MO ("MFMA operand order") copy of the weights feeds the same operands to the same MFMAs as the tiled path's LDS
    turn (ifa_gemm_rows_mfma.hip).  Up to 8 rows both layouts give a wave the same blocks of K: prompts of 3..8 tokens and the
    fused batched step of up to 8 queries must be bit-identical with rows_mo 1 / 0, eager and as a graph replay.  For 9..16
    rows the tiled path walks 2048-column chunks (its LDS also holds the waves' patches) while the MO path stages one
    4096-column chunk: same products, another fp32 summation order -- compared within a tolerance.  test_longffn: w2 rows of
    4352 columns walk two chunks; with the MO copy 2..4 rows are staged whole (CH = 2), 5..8 chunk by chunk -- the same blocks per
    wave in the same order as the tiled path's chunk loop, so still bit-identical up to 8 rows."""
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)
    V = s["vocab"]
    wk.kv_slots(2 * n)
    rng = np.random.default_rng(90 + n)
    prompts = [rng.integers(3, V, 3 + (i * 5) % 6).astype(np.int32) for i in range(n)]
    long_prompt = rng.integers(3, V, 13).astype(np.int32)
    out = {}
    for mo in (1, 0):
        wk.set_option("rows_mo", mo)
        cur, pos = [], []
        for i, pr in enumerate(prompts):
            wk.select_kv(mo * n + i)
            lgp = torch.empty((len(pr), V), dtype=torch.float16, device="cuda")
            cur.append(wk.forward(pr, 0, lgp)); pos.append(len(pr))
            out[(mo, "prompt", i)] = g.host(lgp).copy()
        lg = torch.empty((n, V), dtype=torch.float16, device="cuda")
        for step in range(3):
            slots = list(range(mo * n, mo * n + n))
            t_e = wk.decode_batch(cur, pos, slots, lg)
            out[(mo, "step", step)] = g.host(lg).copy()
            t_g = wk.decode_batch(cur, pos, slots)
            assert [int(t) for t in t_e] == [int(t) for t in t_g]
            out[(mo, "tok", step)] = [int(t) for t in t_e]
            cur = [int(t) for t in t_e]; pos = [p + 1 for p in pos]
        wk.select_kv(mo * n)
        lgl = torch.empty((len(long_prompt), V), dtype=torch.float16, device="cuda")
        wk.forward(long_prompt, 0, lgl)
        out[(mo, "long", 0)] = g.host(lgl).copy()
    for key in [k for k in out if k[0] == 1]:
        a, b = np.asarray(out[key]), np.asarray(out[(0,) + key[1:]])
        if key[1] == "long" or (key[1] == "step" and n > 8):
            a32, b32 = a.astype(np.float32), b.astype(np.float32)
            cos = float((a32 * b32).sum() / (np.linalg.norm(a32) * np.linalg.norm(b32)))
            assert cos >= 0.99999 and np.abs(a32 - b32).max() <= 0.01, (key, cos, np.abs(a32 - b32).max())
        elif not (key[1] == "tok" and n > 8):
            assert np.array_equal(a, b), key
    wk.close()


@pytest.mark.parametrize("T", [2, 5, 8, 11, 16])
@pytest.mark.parametrize("kvd", [dt.F16, dt.Q8_B32T2], ids=["kvf16", "kvq8"])
def test_fused_short_prompt_layer_matches_op_by_op_layer(kvd, T):
    """Prompts of 2..16 tokens run a layer's linears as four launches of the rows GEMM (norm prologue + wq|wk|wv written
    to q / k / v, wo + residual, norm + w1/w3 + GLU, w2 + residual: forward_ops, pf_fused) instead of the op-by-op layer
    (src/transformer/inference_worker.cc:640-1050).  Both at prefix 0 and as the continuation of a cached prefix; the
    cache rows it stores must serve the decode steps that follow."""
    wk, host, s = synth.build("test_mha", dt.Q4_B32T1A, kvd, max_ctx=64, quant_threshold=0, std=0.06, keep_host=True)
    V = s["vocab"]
    wk.kv_slots(2)
    rng = np.random.default_rng(40 + T)
    head = rng.integers(3, V, 7).astype(np.int32)
    for prefix in (0, 7):
        toks = rng.integers(3, V, T).astype(np.int32)
        lg = {}
        nxt = {}
        for slot, fused in ((0, 1), (1, 0)):
            wk.select_kv(slot)
            wk.set_option("batch_fused", 0)
            if prefix:
                wk.forward(head, 0)
            wk.set_option("batch_fused", fused)
            out = torch.empty((T, V), dtype=torch.float16, device="cuda")
            nxt[fused] = wk.forward(toks, prefix, out)
            lg[fused] = g.host(out).astype(np.float32)
        a, b = lg[1], lg[0]
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.9999 and np.abs(a - b).max() <= 0.02, (prefix, cos, np.abs(a - b).max())
        top = np.sort(a[-1])
        if top[-1] - top[-2] > LOGIT_TOL:
            assert nxt[1] == nxt[0]
        # decode on both caches from the same token: the fused layer's cache rows against the op-by-op layer's
        wk.set_option("batch_fused", 1)
        cur = nxt[0]
        for step in range(3):
            outs = []
            for slot in (0, 1):
                wk.select_kv(slot)
                o = torch.empty((1, V), dtype=torch.float16, device="cuda")
                outs.append((wk.forward(np.array([cur], np.int32), prefix + T + step, o), g.host(o).astype(np.float32)))
            # (two caches written by kernels with different summation orders: half-rounding differences of the rows add up)
            da, db = outs[0][1], outs[1][1]
            dcos = float((da * db).sum() / (np.linalg.norm(da) * np.linalg.norm(db)))
            assert dcos >= 0.9998 and np.abs(da - db).max() <= 0.05, (prefix, step, dcos, np.abs(da - db).max())
            cur = outs[1][0]
    wk.close()


def test_1100_token_prompt_two_pass_attention_matches_oracle():
    """Past 1024 keys a chunk of >= 128 queries takes the two-pass attention kernel (csrc/ifa_attn.hip, k_attention_2pass:
    128 queries per workgroup, scores recomputed in the second pass) inside the four-launch prefill layer: the last rows'
    logits of a 1100-token prompt and the decode steps behind it against the oracle."""
    max_ctx = 1152
    wk, host, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=max_ctx, quant_threshold=0, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, dt.F16)
    V = s["vocab"]
    prompt = np.random.default_rng(33).integers(3, V, 1100).astype(np.int32)
    lg = torch.empty((len(prompt), V), dtype=torch.float16, device="cuda")
    tok = wk.forward(prompt, 0, lg)
    tok_orc, lg_orc = om.forward(prompt, 0, nthreads=8)
    a = g.host(lg).astype(np.float32)
    for rows in (slice(0, 64), slice(1000, 1100)):
        cos, mad = _logits_close(a[rows], lg_orc[rows])
        assert cos >= 0.9995 and mad <= 0.03, (rows, cos, mad)
    top = np.sort(lg_orc[-1].astype(np.float32))
    if top[-1] - top[-2] > LOGIT_TOL:
        assert tok == tok_orc
    wk.close()


@pytest.mark.parametrize("kvd,shape,wd", [(dt.F16, "test_gqa", dt.Q4_B32T1A), (dt.Q8_B32T2, "test_gqa", dt.Q4_B32T1A), (dt.F16, "test_moe", dt.Q4_B32T1A),
                                          (dt.Q8_B32T2, "test_gqa", dt.Q3H_B64T1), (dt.F16, "test_gqa", dt.Q4_B64T1)],
                         ids=["kvf16", "kvq8", "moe", "q3h_kvq8", "q4_b64"])
def test_long_prompt_large_tile_layer_matches_oracle_and_op_by_op_layer(kvd, shape, wd):
    """Prompts above 128 tokens run a layer's linears as four launches of the large-tile GEMM (csrc/ifa_gemm.hip, k_gemm_big:
    wq | wk | wv into q / k / v, wo + residual, w1 / w3 + GLU, w2 + residual; forward_ops, pf_big) -- a 170-token prompt and
    a 160-token continuation of it against the oracle (src/transformer/inference_worker.cc:640-1050) and against the
    op-by-op layer of the same library (prefill_big = 0), then decode steps on the cache it wrote.  Mixture-of-experts
    layers: the attention half as two such launches, the expert FFNs device-routed over the rows (moe_ffn).  The 64-weight
    nibble formats (Q3H_B64T1, Q4_B64T1) take the same kernel through a Q4_B32T1A-layout copy of the same values (ensure_x32)."""
    max_ctx = 400
    wk, host, s = synth.build(shape, wd, kvd, max_ctx=max_ctx, quant_threshold=0, std=0.06, keep_host=True)
    om = oracle_model_from_host(host, s, max_ctx, kvd)
    V = s["vocab"]
    prompt = np.random.default_rng(21).integers(3, V, 330).astype(np.int32)
    chunks = [(0, 170), (170, 330)]
    lgs = {}
    for big in (1, 0):
        wk.set_option("prefill_big", big)
        wk.reset()
        outs = []
        for a, b in chunks:
            lg = torch.empty((b - a, V), dtype=torch.float16, device="cuda")
            tok = wk.forward(prompt[a:b], a, lg)
            outs.append((tok, g.host(lg).astype(np.float32)))
        lgs[big] = outs
    moe = shape == "test_moe"
    for ci, (a, b) in enumerate(chunks):
        tok_orc, lg_orc = om.forward(prompt[a:b], a, nthreads=4)
        if moe:
            # a router probability pair closer than the kernels' rounding noise sends a row to another expert (in any of the
            # three implementations): rows are compared one by one and a few such rows are allowed
            for other, tol in ((lg_orc, 0.03), (lgs[0][ci][1], 0.02)):
                rowmax = np.abs(lgs[1][ci][1] - other.astype(np.float32)).max(axis=1)
                assert np.mean(rowmax <= tol) >= 0.96, (ci, tol, np.sort(rowmax)[-8:])
            continue
        cos, mad = _logits_close(lgs[1][ci][1], lg_orc)
        assert cos >= 0.9995 and mad <= 0.03, (ci, cos, mad)
        cos2, mad2 = _logits_close(lgs[1][ci][1], lgs[0][ci][1])
        assert cos2 >= 0.9999 and mad2 <= 0.02, (ci, cos2, mad2)
        top = np.sort(lg_orc[-1].astype(np.float32))
        if top[-1] - top[-2] > LOGIT_TOL:
            assert lgs[1][ci][0] == tok_orc, ci
    if moe:
        wk.close()
        return
    # the op-by-op run came last: rebuild the cache with the large-tile layer, then decode against the oracle
    wk.set_option("prefill_big", 1)
    wk.reset()
    for a, b in chunks:
        cur = wk.forward(prompt[a:b], a)
    toks, _ = wk.decode(cur, len(prompt), 4)
    pos, t_o = len(prompt), cur
    for step in range(4):
        nxt, lg_o = om.forward(np.array([t_o], np.int32), pos, nthreads=4)
        top = np.sort(lg_o[-1].astype(np.float32))
        if top[-1] - top[-2] <= LOGIT_TOL or int(toks[step]) != int(nxt):
            assert top[-1] - top[-2] <= LOGIT_TOL, step
            break
        t_o, pos = int(nxt), pos + 1
    wk.close()


@pytest.mark.parametrize("shape", ["test_moe", "test_moe_longffn"])
@pytest.mark.parametrize("n", [3, 5, 8])
def test_single_row_experts_of_a_batched_moe_step_match_the_grouped_gemv_path(shape, n):
    """The single-row experts of a batched MoE step (csrc/ifa_decode_singles.h: quantiser + tiled-row GEMV + gate in two launches,
    option moe_singles) against the round-3 path (quantiser launches + k_gemv_ax8_grouped on the reference-layout blocks +
    element-wise gate): both are the reference's T = 1 arithmetic for such a row (Q8 activations, int8 dot), so the logits of the
    step must be bit-identical, eager and as a graph replay."""
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)
    V = s["vocab"]
    wk.kv_slots(2 * n)
    rng = np.random.default_rng(300 + n)
    prompts = [rng.integers(3, V, 3 + (i * 5) % 7).astype(np.int32) for i in range(n)]
    cur, pos = [], []
    for i, pr in enumerate(prompts):
        wk.select_kv(i); t = wk.forward(pr, 0)
        wk.select_kv(n + i); assert wk.forward(pr, 0) == t
        cur.append(t); pos.append(len(pr))
    la = torch.empty((n, V), dtype=torch.float16, device="cuda")
    lb = torch.empty((n, V), dtype=torch.float16, device="cuda")
    for step in range(4):
        wk.set_option("moe_singles", 1)
        ta = wk.decode_batch(cur, pos, list(range(n)), la)
        tg = wk.decode_batch(cur, pos, list(range(n)))                       # graph replay of the same step
        # which route the step took: the plan the engine follows for n rows of the fused batched step (the first step built the MO tables)
        for layer in range(s["layers"]):
            p = wk.moe_plan(layer, n, caller_norm=1)
            assert p["kind"] == "device_singles" and p["router"] == "fused" and p["smalls_mo"] == 1 and p["max_tiles"] == 0, p
            assert p["max_smalls"] == min(s["experts"], n) and p["side_stream"] == (1 if p["max_smalls"] > 0 else 0), p
        wk.set_option("moe_singles", 0)
        p = wk.moe_plan(0, n, caller_norm=1)
        assert p["kind"] == "device_grouped" and p["side_stream"] == 0 and p["smalls_mo"] == 1, p
        tb = wk.decode_batch(cur, pos, list(range(n, 2 * n)), lb)
        assert np.array_equal(g.host(la), g.host(lb)), step
        assert [int(t) for t in ta] == [int(t) for t in tb] == [int(t) for t in tg], step
        cur = [int(t) for t in ta]; pos = [p + 1 for p in pos]
    wk.set_option("moe_singles", 1)
    wk.close()
