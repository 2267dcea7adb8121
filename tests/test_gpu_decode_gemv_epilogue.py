"""-m gpu: the epilogue of the fused decode GEMV (k_dec_gemv: lane i finishes row i of a pass) where it chooses a pointer: the output, the
bias and the residual(s) of a row come from scalars of the launch -- set 0's pointer plus the distance of the row's set -- and the values
are requested behind the pass's weights with clamped addresses (an absent vector's request reads a dummy).  What that can get wrong, at
the smallest shapes, against the float64 reference and the bounds of tests/decode_gemv_util.py (docs/decode_gemv_edges.md):

  * the three-set plain QKV launch (option fuse_attn 0), dim 64 and 256, 4 heads of 32, Q4_B32T1A and Q8_B32T2, every combination of a
    bias present or absent on Wq / Wk / Wv (2^3): a bias taken from the wrong set, an absent bias added, a present one dropped, a row
    stored through another set's pointer;
  * one wave's pass on both sides of rows[0] and of rows[0] + rows[1].  A wave's rows are W rows apart (W = the waves of the grid), and
    the grid grows with the rows up to one workgroup per CU: with 4 heads (at most 3 x 4 x 128 rows) no wave of a 256-CU device has a
    second row, so this case -- and only this one -- has W / 64 + 1 heads of 64: every set is 64 rows longer than the grid has waves, a
    wave's consecutive rows lie in consecutive sets and waves 64 and 128 step over the two boundaries inside a pass; the plan of THIS
    device must show it;
  * W2 with and without the second residual (parallel attention adds the layer input), with and without its bias;
  * Wo and W2 with pre_scale / post_scale (attn_out_scale, ffn_out_scale, out_scale), with and without their biases.

Per case: sign inputs (+-1: the norm's output is +-1 whatever its last bit, so the prologue launches are exactly comparable and one wrong row
shows); every launch of the step within max(2 x d_ref, one F16 ulp) of float64; the layer input and every weight and bias tensor unchanged; a
second step bit-identical in every output buffer.  Sentinels: the engine owns its buffers (exact allocations, no frame around them), so
the sentinel pattern is written INTO every output buffer before each step -- an element the launch leaves out keeps it and fails -- and
into nothing else: a store past the last row of an output cannot be seen from here (the q | k | v sections of "dqkv" frame each other: a
row stored through another set's pointer lands on, or is missing from, a checked value)."""
import itertools

import numpy as np
import pytest

from inferflow_amd import dtypes as dt, synth, worker as W
from tests import decode_gemv_util as U

pytestmark = pytest.mark.gpu
TOK = 5
STD = 0.06
SENTINEL = 0x7BCD                      # F16 63904: no output of these inputs comes near it
FORMATS = (dt.Q4_B32T1A, dt.Q8_B32T2)
ID = {d: dt.name(d).lower() for d in FORMATS}
BIAS = {W.T_WQ: W.T_WQ_B, W.T_WK: W.T_WK_B, W.T_WV: W.T_WV_B, W.T_WO: W.T_WO_B, W.T_W1: W.T_W1_B, W.T_W3: W.T_W3_B, W.T_W2: W.T_W2_B}
NAMES = {W.T_WQ: "wq", W.T_WK: "wk", W.T_WV: "wv", W.T_WO: "wo", W.T_W1: "w1", W.T_W3: "w3", W.T_W2: "w2"}
OUTS = dict(qkv="dqkv", wo="a", ffn13="t1", w2="x2")


def _build(wd, dim, heads, head_dim, ffn, biased=(), **cfg):
    """a one-layer model with every matrix in format wd and a bias on the matrices named in `biased`; -> (worker, cfg, Model, raw tensors)"""
    import torch
    s = dict(dim=dim, layers=1, heads=heads, kv_heads=heads, head_dim=head_dim, ffn=ffn, vocab=64)
    wk = W.DecodeWorker(max_ctx=8, kv_dtype=dt.F16, **s, **cfg)
    dev = "cuda:0"
    ones = torch.ones(dim, dtype=torch.float16, device=dev)
    wk.set_tensor_f16(-1, W.T_EMBD, dt.F16, synth.gen_f16((64, dim), 999, STD, dev))
    wk.set_tensor_f16(-1, W.T_OUT_NORM, dt.F16, ones)
    wk.set_tensor_f16(-1, W.T_LM_HEAD, dt.F16, synth.gen_f16((64, dim), 998, STD, dev))
    wk.set_tensor_f16(0, W.T_ATTN_NORM, dt.F16, ones)
    if not cfg.get("parallel_attn"):
        wk.set_tensor_f16(0, W.T_FFN_NORM, dt.F16, ones)
    for tid, kind in synth.MATRICES:
        rows, cols = synth._shape(kind, s)
        wk.set_tensor_f16(0, tid, wd, synth.gen_f16((rows, cols), 1000 + tid, STD, dev), rows, cols)
        if tid in biased:      # (std 0.5: a bias lost, doubled or taken from another set is far outside any bound)
            wk.set_tensor_f16(0, BIAS[tid], dt.F16, synth.gen_f16((rows,), 2000 + tid, 0.5, dev))
    wk.finalize()
    ok, why = wk.fused_supported()
    assert ok, why
    for k, v in (("fuse_attn", 0), ("fuse_ffn", 0), ("step_tail", 0), ("debug_hidden_in", 1)):
        wk.set_option(k, v)
    raw = {tid: wk.get_tensor_host(0, tid) for tid in list(BIAS) + list(BIAS.values())}
    mats = {}
    for tid, btid in BIAS.items():
        d, data, rows, cols = raw[tid]
        assert (raw[btid] is not None) == (tid in biased), ("bias tensors of the model differ from the case's", tid)
        mats[NAMES[tid]] = U.Mat(d, data, rows, cols, bias=raw[btid][1].view(np.float16) if raw[btid] is not None else None)
    full = dict(s, **cfg)
    ones_h = np.ones(dim, np.float16)
    model = U.Model(full, mats, dict(attn_norm=ones_h, ffn_norm=None if cfg.get("parallel_attn") else ones_h))
    return wk, full, model, raw


def _run(wk, model, x16, where, roles):
    """the sentinel pattern into every output buffer, one step at position 0, twice: -> the buffers of the first step, checked"""
    got = []
    for rep in range(2):
        for name in OUTS.values():
            n = wk.buffer(name)[1]
            wk.write_buffer(name, np.full(n // 2, SENTINEL, np.uint16))
        wk.write_buffer("x", x16.view(np.uint16))
        wk.decode(TOK, 0, 1)
        got.append({n: wk.read_buffer(n).copy() for n in ("x", "dqkv", "att", "attq", "a", "t1", "x2") if wk.buffer(n)[1] > 0})
    bufs, again = got
    assert np.array_equal(bufs["x"].view(np.uint16), x16.view(np.uint16)), ("the layer input changed", where)
    for name in OUTS.values():
        assert not (bufs[name].view(np.uint16) == SENTINEL).any(), ("an element of %s was not written" % name, where)
        assert np.array_equal(bufs[name], again[name]), ("a second step differs in %s" % name, where)
    launches, _ = U.step_launches(model, x16, bufs, "sign", wk.gemv_plan(0, "wo")["norm"] == 2)
    for role in roles:
        L = launches[role]
        assert L.exact, (where, role)
        med, worst = U.check_exact(bufs[OUTS[role]].view(np.float16), L)
        print("decode-gemv-epilogue %-44s %-5s rows %5d  err / bound median %.3f worst %.3f" % (where, role, L.rows, med, worst))
    return bufs


def _unchanged(wk, raw, where):
    for tid, v in raw.items():
        now = wk.get_tensor_host(0, tid)
        assert (v is None) == (now is None) and (v is None or np.array_equal(v[1], now[1])), ("a weight or bias tensor changed", where, tid)


def _sign(cols):
    return U.make_input("sign", cols, dt.Q4_B32T1A, U.seed_of(cols))


@pytest.mark.parametrize("wd", FORMATS, ids=[ID[d] for d in FORMATS])
def test_qkv_bias_on_every_combination_of_sets(wd):
    for dim, combo in itertools.product((64, 256), itertools.product((False, True), repeat=3)):
        biased = [t for t, on in zip((W.T_WQ, W.T_WK, W.T_WV), combo) if on]
        where = "%s dim %d bias q k v %s" % (ID[wd], dim, "".join("+" if b else "-" for b in combo))
        wk, cfg, model, raw = _build(wd, dim, 4, 32, 256, biased=biased, attn_out_scale=1e-12)
        p = wk.gemv_plan(0, "qkv")
        assert (p["single"], p["error"], p["kind"], p["total_rows"], p["epi"], p["norm"]) == (1, 0, "classic", 3 * 128, U.EPI_PLAIN, 1), (where, p)
        _run(wk, model, _sign(dim), where, ("qkv",))
        _unchanged(wk, raw, where)
        wk.close()


@pytest.mark.parametrize("wd", FORMATS, ids=[ID[d] for d in FORMATS])
def test_one_pass_of_a_wave_on_both_sides_of_the_set_boundaries(wd):
    probe, _, _, _ = _build(wd, 64, 4, 32, 256)
    pp = probe.gemv_plan(0, "qkv")
    probe.close()
    w_full = pp["num_cus"] * pp["threads"] // 64            # the waves of a full grid
    heads = w_full // 64 + 1                                # 64 rows each: every set has 64 rows more than the grid has waves
    for combo in ((True, True, True), (True, False, True), (False, True, False)):
        biased = [t for t, on in zip((W.T_WQ, W.T_WK, W.T_WV), combo) if on]
        where = "%s %d heads of 64, bias q k v %s" % (ID[wd], heads, "".join("+" if b else "-" for b in combo))
        wk, cfg, model, raw = _build(wd, 64, heads, 64, 256, biased=biased, attn_out_scale=1e-12)
        p = wk.gemv_plan(0, "qkv")
        waves, rset = p["grid"] * p["threads"] // 64, heads * 64
        assert (p["single"], p["error"], p["kind"], p["epi"], p["norm"]) == (1, 0, "classic", U.EPI_PLAIN, 1), (where, p)
        assert waves == w_full and p["total_rows"] == 3 * rset and p["rw"] >= 2, (where, p)
        # row (pass x rw + i) x waves + wave: some wave's pass has rows of two sets, on either side of rows[0] and of rows[0] + rows[1]
        crossed = set()
        for wave, ps in itertools.product((0, 63, 64, 127, 128), range(p["npass"])):
            rows = [(ps * p["rw"] + i) * waves + wave for i in range(p["rw"])]
            crossed |= {(a // rset, b // rset) for a, b in zip(rows, rows[1:]) if b < 3 * rset and a // rset != b // rset}
        assert {(0, 1), (1, 2)} <= crossed, (where, crossed)
        _run(wk, model, _sign(64), where, ("qkv",))
        _unchanged(wk, raw, where)
        wk.close()


@pytest.mark.parametrize("wd", FORMATS, ids=[ID[d] for d in FORMATS])
def test_w2_with_and_without_the_second_residual(wd):
    for par, bias in itertools.product((0, 1), (False, True)):
        where = "%s parallel_attn %d w2 bias %d" % (ID[wd], par, bias)
        wk, cfg, model, raw = _build(wd, 128, 4, 32, 256, biased=[W.T_W2, W.T_WO] if bias else [], **(dict(parallel_attn=1) if par else {}))
        p = wk.gemv_plan(0, "w2")
        assert (p["single"], p["error"], p["epi"], p["norm"], p["total_rows"]) == (1, 0, U.EPI_RESIDUAL, 0, 128), (where, p)
        assert wk.gemv_plan(0, "wo")["epi"] == (U.EPI_PLAIN if par else U.EPI_RESIDUAL), where
        _run(wk, model, _sign(128), where, ("wo", "w2"))
        _unchanged(wk, raw, where)
        wk.close()


@pytest.mark.parametrize("wd", FORMATS, ids=[ID[d] for d in FORMATS])
def test_wo_and_w2_with_pre_and_post_scale(wd):
    for scales, bias in itertools.product((dict(attn_out_scale=0.25, ffn_out_scale=0.5), dict(attn_out_scale=0.25, ffn_out_scale=0.5, out_scale=1.5),
                                           dict(out_scale=0.75)), (False, True)):
        where = "%s %s bias %d" % (ID[wd], " ".join("%s %g" % kv for kv in scales.items()), bias)
        wk, cfg, model, raw = _build(wd, 256, 4, 32, 64, biased=[W.T_WO, W.T_W2] if bias else [], **scales)
        for role in ("wo", "w2"):
            p = wk.gemv_plan(0, role)
            assert (p["single"], p["error"], p["epi"]) == (1, 0, U.EPI_RESIDUAL), (where, role, p)
        _run(wk, model, _sign(256), where, ("wo", "w2"))
        _unchanged(wk, raw, where)
        wk.close()
