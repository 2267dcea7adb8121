"""-m gpu: the int8 rows GEMM (k_gemm_rows_i8; docs/rows_gemm_int8.md) through ifa_gemm_rows_q8 and, with option rows_i8, the batched step.
A. Every output row t is BIT-EQUAL to the single-token ops: ifa_gemv_tiled on ifa_quantize_act_q8 of row t (ifa_layernorm in front when
   norm = 1), then ifa_add (residual) or ifa_activation_mul (gated pair: Activation -> F16, Mul -> F16 -- the op-by-op layer's call and the
   decode GEMV's EPI_GLU; ifa_activation with is_glu rounds once and differs in 201 of 816 elements at K 128, T 17, N 48 on MI355X).
B. Every element is within a derived bound of float64 math on the device's codes, y = sum_b xs_b (dot_b scale_b + xsum_b base_b): fp32
   accumulation of nblk terms in any order errs by at most nblk 2^-24 sum_b |term_b|, and every F16 rounding of the path (the sum, + bias,
   res + y, or act -- slope <= 1.1 -- and the product) by at most half an F16 ulp of its value.
Every case runs planned for the device (one tile per workgroup at these sizes) and for ONE CU: a workgroup then walks all the tiles of the
launch (2..4; the sets meet inside it), the path of every launch of a real model.
Nothing outside [T][N] of the output frame may be written."""
import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth, worker as W
from tests import gpu_util as g
from tests import prompt_gemm_util as P
from tests import rows_gemm_util as U
from tests.decode_attn_util import ulp16

pytestmark = pytest.mark.gpu
PLAIN, RESIDUAL, GLU = U.PLAIN, U.RESIDUAL, U.GLU
# (K, T, rows, epilogue, norm, bias, inputs).  K 128: 4 live classes, 2048: each once, 2176: classes 0..3 twice; T: both token tiles ragged / full
CASES = [
    (128, 2, (16,), PLAIN, 0, False, "dense"), (128, 16, (40,), RESIDUAL, 0, True, "dense"), (128, 17, (48,), GLU, 1, False, "dense"),
    (2048, 3, (40,), PLAIN, 1, True, "dense"), (2048, 17, (48,), GLU, 0, True, "dense"), (2048, 32, (16, 16, 32), PLAIN, 1, False, "dense"),
    (2176, 16, (16, 16, 32), PLAIN, 0, True, "dense"), (2176, 32, (48,), GLU, 1, True, "dense"), (2176, 3, (16,), RESIDUAL, 1, False, "dense"),
    (4224, 17, (40,), RESIDUAL, 0, False, "dense"), (4224, 32, (16, 16, 32), PLAIN, 0, False, "dense"), (4224, 2, (48,), GLU, 0, False, "dense"),
    (2048, 3, (16,), PLAIN, 0, False, "zero_row"), (2176, 2, (40,), PLAIN, 0, True, "last_block"),
]


def _case_id(c):
    return "K%d-T%d-N%s-epi%d-norm%d%s-%s" % (c[0], c[1], "+".join(map(str, c[2])), c[3], c[4], "-bias" if c[5] else "", c[6])


def _inputs(K, T, rows, epi, bias, family):
    rng = np.random.default_rng(K + 7 * T + 13 * sum(rows) + 101 * epi)
    x = U.make_rows("dense", T, K, 5 + K + T)
    if family == "zero_row":
        x[1] = 0
    if family == "last_block":          # one live block, the last one of the second round of class 3
        x[:, :K - 32] = 0
    mats = [P.Mat(dt.Q4_B32T1A, U._quantized(dt.Q4_B32T1A, r, K, 40 + K + i), r, K, rng.normal(0, U.B_STD, r).astype(np.float16) if bias else None)
            for i, r in enumerate(rows + (rows[:1] if epi == GLU else ()))]
    res = rng.normal(0, 1, (T, sum(rows))).astype(np.float16) if epi == RESIDUAL else None
    return x, mats[:len(rows)], (mats[-1] if epi == GLU else None), res


def _f64(xq, mats):
    T = xq.shape[0]
    blocks = xq.reshape(T, -1, 34)
    xs = blocks[:, :, :2].copy().view(np.float16).astype(np.float64).reshape(T, -1)
    xc = blocks[:, :, 2:].view(np.int8).astype(np.float64)
    ys, mags = [], []
    for m in mats:
        q, base, scale = P.codes_and_words(m.dtype, m.data, m.cols)
        dot = np.einsum("tbk,nbk->tnb", xc, q.reshape(m.rows, -1, 32).astype(np.float64))
        term = xs[:, None, :] * (dot * scale[None].astype(np.float64) + xc.sum(-1)[:, None, :] * base[None].astype(np.float64))
        ys.append(term.sum(-1))
        mags.append(np.abs(term).sum(-1) * xs.shape[1] * 2.0 ** -24)
    y, e = np.concatenate(ys, 1), np.concatenate(mags, 1)
    e = e + 0.5 * ulp16(np.abs(y))
    if mats[0].bias is not None:
        y = y + np.concatenate([m.bias for m in mats]).astype(np.float64)[None]
        e = e + 0.5 * ulp16(np.abs(y))
    return y, e


@pytest.mark.parametrize("num_cus", (0, 1))
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_rows_equal_decode_gemv(case, num_cus):
    K, T, rows, epi, norm, bias, family = case
    N, lib, s = sum(rows), g.capi(), g.stream()
    x, mats, w3, res = _inputs(K, T, rows, epi, bias, family)
    xd, nw = g.dev(x), g.dev(U.norm_weight(K))
    wt = [g.repack(m.dtype, g.dev(m.data), m.rows, K) for m in mats]
    w3t = g.repack(w3.dtype, g.dev(w3.data), w3.rows, K) if w3 is not None else None
    bd = [g.dev(m.bias) if bias else None for m in mats]
    b3 = g.dev(w3.bias) if w3 is not None and bias else None
    resd = g.dev(res) if res is not None else None
    # ---- the launch under test, into sentinel frames (three sets: one frame per set, Yset)
    widths = rows if len(rows) > 1 else (N,)
    frames = [g.dev(P.sentinel_frame(T, n, n + 8)) for n in widths]
    rc = W.gemm_rows_q8(dt.Q4_B32T1A, [g.p(t) for t in wt], rows, K, g.p(xd), T, y=g.p(frames[0]), ldy=N + 8,
                        yset=[g.p(f) for f in frames] if len(rows) > 1 else None, epi=epi, norm=norm, norm_w=g.p(nw), eps=1e-5,
                        bias=[g.p(b) for b in bd] if bias else None, w1=g.p(w3t), bias1=g.p(b3), res=g.p(resd), ldres=N, num_cus=num_cus, stream=s)
    ia.check(rc)
    xin = xd
    if norm:
        xin = g.empty_f16(T, K)
        ia.check(lib.ifa_layernorm(0, g.p(xd), T, K, g.p(nw), None, 0.0, 1e-5, g.p(xin), s))
    xq = g.quantize_act(xin)
    gemv = lambda t: torch.stack([torch.cat([g.gemv_tiled(m.dtype, w, m.rows, K, xq[r], b) for m, w, b in t]) for r in range(T)])
    want = gemv(list(zip(mats, wt, bd)))
    if epi == RESIDUAL:
        ia.check(lib.ifa_add(g.p(resd), g.p(want.clone()), T * N, 0, g.p(want), s))
    if epi == GLU:
        ia.check(lib.ifa_activation_mul(0, g.p(want.clone()), g.p(gemv([(w3, w3t, b3)])), T * N, g.p(want), s))
    g.sync()
    if len(rows) > 1:
        got = np.concatenate([g.host(f).reshape(-1)[:T * n].reshape(T, n) for f, n in zip(frames, rows)], 1).view(np.float16)
        for f, n in zip(frames, rows):
            assert np.array_equal(g.host(f).view(np.uint16).reshape(-1)[T * n:], P.sentinel_frame(T, n, n + 8).reshape(-1)[T * n:]), "written past a set's rows"
    else:
        P.check_sentinel(g.host(frames[0]), T, N, N + 8, _case_id(case))
        got = g.host(frames[0]).view(np.float16)[:T, :N]
    want = g.host(want)
    diff = got.view(np.uint16) != want.view(np.uint16)
    assert not diff.any(), "%d of %d elements differ from the single-token ops, first at %s" % (diff.sum(), diff.size, np.argwhere(diff)[0])
    xqh = g.host(xq)
    y, e = _f64(xqh, mats)
    if epi == RESIDUAL:
        y = res.astype(np.float64) + y
        e = e + 0.5 * ulp16(np.abs(y))
    if epi == GLU:
        y3, e3 = _f64(xqh, [w3])
        act = y / (1.0 + np.exp(-y))
        ea = 1.1 * e + 0.5 * ulp16(np.abs(act))
        y, e = act * y3, np.abs(y3) * ea + np.abs(act) * e3 + ea * e3
        e = e + 0.5 * ulp16(np.abs(y))
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= e).all(), "worst error / bound %.3f at %s" % (float((err / e).max()), np.unravel_index(np.argmax(err / e), err.shape))


# ----------------------------------------------------------------------------- the batched step with the option
@pytest.fixture(scope="module")
def models():
    build = lambda: synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=8, quant_threshold=0, std=0.06)
    (wk, _, s), (plain, _, _) = build(), build()
    wk.kv_slots(32)
    plain.kv_slots(32)
    return wk, plain, s


def _step(wk, s, tokens):
    n = len(tokens)
    logits = torch.zeros((n, s["vocab"]), dtype=torch.float16, device="cuda:0")
    W.gemm_rows_launches()
    wk.decode_batch(tokens, [0] * n, list(range(n)), logits_out=logits)
    return g.host(logits).view(np.uint16), W.gemm_rows_launches()[1]


def test_batched_step_rows_do_not_depend_on_partners(models):
    wk, plain, s = models
    q, fused = 5, 4 * s["layers"]
    others = [(3 * i + 1) % s["vocab"] for i in range(16)]
    base, n_off = _step(plain, s, [q] + others[:1])
    assert n_off >= fused, "the step must take the fused route: four k_gemm_rows_mfma launches per layer"
    wk.set_option("rows_i8", 1)
    two, n_on = _step(wk, s, [q] + others[:1])
    assert n_on == n_off - fused, "with rows_i8 the four launches of every layer of this model run k_gemm_rows_i8"
    for at in (0, 7, 16):
        many, n_on = _step(wk, s, others[:at] + [q] + others[at:])
        assert np.array_equal(many[at], two[0]), "row %d of 17 differs from the row with one partner" % at
    # a batched row and a draft row against the single-token step (same token, position, cache): the last layer's attention output, wo +
    # residual and gated product are the same bits; the logits are not compared (the lm_head of a batched step is not a rows-GEMM launch)
    wk.select_kv(0)
    wk.decode(q, 0, 1)
    single = {k: wk.read_buffer(k).view(np.uint16).copy() for k in ("att", "a", "t1")}
    for step in (lambda: wk.decode_batch([q] + others[:1], [0, 0], [0, 1]), lambda: wk.decode_draft([q] + others[:2], 0)):
        step()
        for k, v in single.items():
            assert np.array_equal(wk.read_buffer("rows_" + k).view(np.uint16)[:v.size], v), "%s of row 0 differs from the single-token step" % k
    wk.forward(others[:5], 0)
    assert wk.prompt_route()["kind"] == "rows", "a 5-token prompt must still report the rows route"
    wk.set_option("rows_i8", 0)
    off, n_now = _step(wk, s, [q] + others[:1])
    assert n_now == n_off and np.array_equal(off, base), "rows_i8 = 0 is not the path of a model that never had the option"
