"""-m gpu: the draft step at the worker level (ifa_model_decode_draft, csrc/ifa_decode_draft_kv.hip): n rows of ONE slot in one batched
step, row i behind cache rows [0, pos0 + i).  Each row is bit for bit -- logits, id, the K / V row it writes -- the row
ifa_model_decode_batch computes for an independent query whose slot holds the same bytes; nothing is written past the n rows; the
graph replay gives the eager ids; the fused route agrees with the op-by-op one inside the bound between the two batched routes;
rows of rejected drafts leave no trace in later steps; the refusals are error codes."""
import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth
from tests import gpu_util as g

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.03      # tests/test_gpu_engine.py
KV = [("test_gqa", dt.F16), ("test_gqa", dt.Q8_B32T2), ("test_mha", dt.F16), ("test_mha", dt.Q8_B32T2)]
KV_IDS = ["%s-%s" % (s, "f16" if k == dt.F16 else "q8") for s, k in KV]
# (n rows, max_ctx, prompt tokens): the short prompt stays inside one wave of keys; 253 + 5 rows straddle the 256-row entry prefetch
GEOM = [(2, 64, 11), (5, 64, 11), (8, 64, 11), (5, 720, 253)]


class Model:
    """one worker per (shape, cache type, max_ctx): 8 slots, slot 0 prefilled; snapshot() / restore() put slot 0 back"""

    def __init__(self, shape, kvd, max_ctx, n_prompt):
        self.wk, _, self.s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=max_ctx, quant_threshold=0, std=0.06)
        self.wk.kv_slots(8)
        self.V, self.layers, self.max_ctx = self.s["vocab"], self.s["layers"], max_ctx
        self.rb = dt.row_bytes(kvd, self.s["kv_heads"] * self.s["head_dim"])
        rng = np.random.default_rng(41)
        self.prompt = rng.integers(3, self.V, n_prompt).astype(np.int32)
        self.drafts = rng.integers(3, self.V, 16).astype(np.int32)
        self.wk.select_kv(0)
        self.t0 = int(self.wk.forward(self.prompt, 0))
        self.pos0 = n_prompt
        self.snap = self.read_slot(0)

    def read_slot(self, slot):
        self.wk.select_kv(slot)
        out = [(self.wk.read_buffer("kcache", l).copy(), self.wk.read_buffer("vcache", l).copy()) for l in range(self.layers)]
        return out

    def restore(self):
        self.wk.set_option("batch_fused", 1)
        self.wk.select_kv(0)
        for l, (k, v) in enumerate(self.snap):
            self.wk.write_buffer("kcache", k, l)
            self.wk.write_buffer("vcache", v, l)

    def logits(self, n):
        return torch.empty((n, self.V), dtype=torch.float16, device="cuda")


_MODELS = {}


def _model(shape, kvd, max_ctx, n_prompt):
    key = (shape, kvd, max_ctx, n_prompt)
    if key not in _MODELS:
        _MODELS[key] = Model(*key)
    m = _MODELS[key]
    m.restore()
    return m


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.wk.close()
    _MODELS.clear()


def _bits(t):
    return g.host(t).view(np.uint16).copy()


@pytest.mark.parametrize("n,max_ctx,n_prompt", GEOM, ids=["n2", "n5", "n8", "n5-bucket-edge"])
@pytest.mark.parametrize("shape,kvd", KV, ids=KV_IDS)
def test_rows_are_bit_identical_to_independent_queries(shape, kvd, n, max_ctx, n_prompt):
    m = _model(shape, kvd, max_ctx, n_prompt)
    wk, pos0, rb = m.wk, m.pos0, m.rb
    toks = np.concatenate([[m.t0], m.drafts[:n - 1]]).astype(np.int32)
    lgd, lgb = m.logits(n), m.logits(n)
    wk.select_kv(0)
    ids_d = wk.decode_draft(toks, pos0, lgd)
    after = m.read_slot(0)
    lo, hi = pos0 * rb, (pos0 + n) * rb
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(after[l][kv][:lo], m.snap[l][kv][:lo]), (l, kv, "rows in front of the step")
            assert np.array_equal(after[l][kv][hi:], m.snap[l][kv][hi:]), (l, kv, "bytes past row pos0 + n - 1")
            for i in range(n):
                assert after[l][kv][lo + i * rb:lo + (i + 1) * rb].any(), (l, kv, i, "row not written")
    for i in range(1, n):
        wk.kv_copy(0, i, pos0 + n)
    wk.sync()
    ids_b = wk.decode_batch(toks, [pos0 + i for i in range(n)], list(range(n)), lgb)
    assert [int(t) for t in ids_d] == [int(t) for t in ids_b]
    assert np.array_equal(_bits(lgd), _bits(lgb))
    for i in range(n):
        got = m.read_slot(i)
        a, b = (pos0 + i) * rb, (pos0 + i + 1) * rb
        for l in range(m.layers):
            for kv in (0, 1):
                assert np.array_equal(got[l][kv][a:b], after[l][kv][a:b]), (i, l, kv)


@pytest.mark.parametrize("shape,kvd", KV, ids=KV_IDS)
def test_graph_replay_returns_the_eager_ids(shape, kvd):
    n = 5
    m = _model(shape, kvd, 64, 11)
    toks = np.concatenate([[m.t0], m.drafts[:n - 1]]).astype(np.int32)
    m.wk.select_kv(0)
    eager = [int(t) for t in m.wk.decode_draft(toks, m.pos0, m.logits(n))]
    for _ in range(2):      # capture, then replay
        assert [int(t) for t in m.wk.decode_draft(toks, m.pos0)] == eager


def _fused_against_op_by_op(wk, V, toks, pos0, n):
    """slot 0 fused, slot 1 (a copy of its rows) op-by-op: the bounds of test_fused_batched_step_matches_op_by_op_rows_and_graph_replay"""
    wk.kv_copy(0, 1, pos0)
    wk.sync()
    lgf = torch.empty((n, V), dtype=torch.float16, device="cuda")
    lgu = torch.empty((n, V), dtype=torch.float16, device="cuda")
    wk.set_option("batch_fused", 1)
    wk.select_kv(0)
    tf = wk.decode_draft(toks, pos0, lgf)
    wk.set_option("batch_fused", 0)
    wk.select_kv(1)
    tu = wk.decode_draft(toks, pos0, lgu)
    tg = wk.decode_draft(toks, pos0)            # the op-by-op rows as a graph of their own
    wk.set_option("batch_fused", 1)
    assert [int(t) for t in tg] == [int(t) for t in tu]
    a, b = g.host(lgf).astype(np.float32), g.host(lgu).astype(np.float32)
    cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
    print("fused vs op-by-op draft step: cos %.7f max|d| %.5f" % (cos, np.abs(a - b).max()))
    assert cos >= 0.9999 and np.abs(a - b).max() <= 0.02, (cos, np.abs(a - b).max())
    gaps = np.sort(a, axis=1)
    for i in range(n):
        if gaps[i, -1] - gaps[i, -2] > LOGIT_TOL:
            assert int(tf[i]) == int(tu[i]), i


@pytest.mark.parametrize("shape,kvd", KV, ids=KV_IDS)
def test_fused_route_against_op_by_op_route(shape, kvd):
    n = 5
    m = _model(shape, kvd, 64, 11)
    toks = np.concatenate([[m.t0], m.drafts[:n - 1]]).astype(np.int32)
    _fused_against_op_by_op(m.wk, m.V, toks, m.pos0, n)


def test_fused_route_against_op_by_op_route_moe():
    n = 5
    wk, _, s = synth.build("test_moe", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    wk.kv_slots(2)
    rng = np.random.default_rng(43)
    prompt = rng.integers(3, s["vocab"], 11).astype(np.int32)
    wk.select_kv(0)
    t0 = int(wk.forward(prompt, 0))
    toks = np.concatenate([[t0], rng.integers(3, s["vocab"], n - 1)]).astype(np.int32)
    _fused_against_op_by_op(wk, s["vocab"], toks, len(prompt), n)
    wk.close()


@pytest.mark.parametrize("shape,kvd", KV, ids=KV_IDS)
def test_rejected_rows_do_no_harm(shape, kvd):
    n = 5
    m = _model(shape, kvd, 64, 11)
    wk, pos0, rb = m.wk, m.pos0, m.rb
    wrong = np.concatenate([[m.t0], m.drafts[:n - 1]]).astype(np.int32)
    wk.select_kv(0)
    first = wk.decode_draft(wrong, pos0)
    nxt = int(first[0])
    assert any(int(first[i]) != int(wrong[i + 1]) for i in range(n - 1)), "the drafts were meant to be wrong"
    wk.kv_copy(0, 1, pos0 + 1)                 # the twin: only the rows that count, never the rejected ones
    wk.sync()
    toks = np.concatenate([[nxt], m.drafts[8:8 + n - 1]]).astype(np.int32)
    lga, lgb = m.logits(n), m.logits(n)
    wk.select_kv(0)
    ia_ = wk.decode_draft(toks, pos0 + 1, lga)
    wk.select_kv(1)
    ib_ = wk.decode_draft(toks, pos0 + 1, lgb)
    assert [int(t) for t in ia_] == [int(t) for t in ib_]
    assert np.array_equal(_bits(lga), _bits(lgb))
    sa, sb = m.read_slot(0), m.read_slot(1)
    end = (pos0 + 1 + n) * rb
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(sa[l][kv][:end], sb[l][kv][:end]), (l, kv)


def test_refusals_are_error_codes():
    m = _model("test_gqa", dt.F16, 64, 11)
    L, h = ia.lib(), m.wk._h
    toks = np.concatenate([[m.t0], m.drafts[:8]]).astype(np.int32)
    out = np.zeros(16, np.int32)
    tp, op = toks.ctypes.data, out.ctypes.data
    m.wk.select_kv(0)
    for n, pos0 in ((1, m.pos0), (9, m.pos0), (0, m.pos0), (5, m.max_ctx - 4), (2, m.max_ctx - 1), (5, -1)):
        assert L.ifa_model_decode_draft(h, n, tp, pos0, op, None) == -1, (n, pos0)
        assert b"ifa_model_decode_draft" in L.ifa_last_error()
    assert L.ifa_model_decode_draft(h, 5, None, m.pos0, op, None) == -1
    assert L.ifa_model_decode_draft(h, 5, tp, m.max_ctx - 5, op, None) == 0            # the last rows of the cache are in range
    m.restore()
    m.wk.set_option("exact_order", 1)
    assert L.ifa_model_decode_draft(h, 5, tp, m.pos0, op, None) == -4 and b"exact_order" in L.ifa_last_error()
    m.wk.set_option("exact_order", 0)
    m.wk.set_option("perf_stat", 1)
    assert L.ifa_model_decode_draft(h, 5, tp, m.pos0, op, None) == -4 and b"perf_stat" in L.ifa_last_error()
    m.wk.set_option("perf_stat", 0)
    after = m.read_slot(0)                      # the refused calls wrote nothing
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(after[l][kv], m.snap[l][kv]), (l, kv)
    assert [int(t) for t in m.wk.decode_draft(toks[:5], m.pos0)] == [int(t) for t in m.wk.decode_draft(toks[:5], m.pos0, m.logits(5))]
