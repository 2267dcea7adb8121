"""-m gpu: the sampled draft step at the worker level (ifa_model_decode_draft_sampled, csrc/ifa_engine_draft_sampled.hip).  After each
call the step's n logits rows ("logits", or "logits_adj" for a processed query) are read back: their pools (pool_ref) through
ifa_sample_verify_host must give the call's tokens, n_out and generator state.  The cache rows are those of ifa_model_decode_draft
on the same tokens; full acceptance is built deterministically; greedy accepts where ifa_model_decode_draft's ids equal the drafts;
the logit state is never written; the other steps' graphs survive; the refusals carry their messages."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import _capi, dtypes as dt, synth
from inferflow_amd import worker as W
from tests.pool_util import pool_ref

pytestmark = pytest.mark.gpu

MAX_CTX, N_PROMPT, POOL = 64, 11, 50
BIAS = {17: -100.0, 400: float("-inf")}


def _params(strategy=4, temperature=0.9, top_p=0.9, max_k=8, min_p=0.05, pool=POOL):
    return _capi.SampleParams(strategy, temperature, top_p, max_k, min_p, pool)


class Model:
    def __init__(self, kvd):
        self.wk, _, self.s = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=MAX_CTX, quant_threshold=0, std=0.06)
        self.V, self.layers = self.s["vocab"], self.s["layers"]
        rng = np.random.default_rng(41)
        self.prompt = rng.integers(3, self.V, N_PROMPT).astype(np.int32)
        self.junk = rng.integers(3, self.V, 16).astype(np.int32)
        self.t0 = int(self.wk.forward(self.prompt, 0))
        self.pos0 = N_PROMPT
        self.snap = self.kv()

    def kv(self):
        return [self.wk.read_buffer(n, l).copy() for l in range(self.layers) for n in ("kcache", "vcache")]

    def restore(self):
        for i, b in enumerate(self.snap):
            self.wk.write_buffer(("kcache", "vcache")[i % 2], b, i // 2)

    def arm(self):
        """the processors of slot 0: the prompt marked, the first token counted"""
        self.wk.logit_state_reset(0, self.prompt, rep=1.3, freq=0.25, pres=0.5, bias={**BIAS, int(self.prompt[0]): 5.0})
        self.wk.logit_state_add([0], [self.t0])
        self.wk.sync()

    def state(self):
        return self.wk.read_buffer("logit_state", nbytes=self.V * 4).view(np.uint32).copy()


_MODELS = {}


def _model(kvd):
    if kvd not in _MODELS:
        _MODELS[kvd] = Model(kvd)
    _MODELS[kvd].restore()
    return _MODELS[kvd]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.wk.close()
    _MODELS.clear()


def _call(m, toks, p, st, slot=-1):
    """one call, checked against the host chain on the pools of the rows the step left behind; returns (tokens, state)"""
    toks = np.asarray(toks, np.int32)
    n = toks.size
    out, st_new = m.wk.decode_draft_sampled(toks, m.pos0, p, st, slot)
    rows = m.wk.read_buffer("logits_adj" if slot >= 0 else "logits", nbytes=n * m.V * 2).view(np.float16).reshape(n, m.V)
    k = p.pool_size
    counts, ids, vals = np.zeros(n, np.int32), np.zeros((n, k), np.int32), np.zeros((n, k), np.uint16)
    for i in range(n):
        pid, bits = pool_ref(rows[i], k)
        counts[i] = len(pid)
        ids[i, :len(pid)] = pid
        vals[i, :len(pid)] = bits
    want_toks, _, want_n, want_st, err = W.sample_verify_host(counts, ids, vals, p, toks[1:], st)
    assert err == 0
    assert ([int(t) for t in out], st_new) == ([int(t) for t in want_toks[:want_n]], want_st), (out, want_toks, want_n)
    return [int(t) for t in out], st_new


KVD = [dt.F16, dt.Q8_B32T2]
KVD_IDS = ["f16", "q8"]


@pytest.mark.parametrize("kvd", KVD, ids=KVD_IDS)
@pytest.mark.parametrize("n", [2, 5, 8])
def test_cache_rows_are_those_of_the_greedy_draft_step(kvd, n):
    m = _model(kvd)
    toks = np.concatenate([[m.t0], m.junk[:n - 1]]).astype(np.int32)
    m.wk.decode_draft(toks, m.pos0)
    want = m.kv()
    m.restore()
    out, st = _call(m, toks, _params(), W.rng_state_of_seed(7))
    assert 1 <= len(out) <= n and st == _advance(W.rng_state_of_seed(7), 2 * len(out))
    for a, b in zip(m.kv(), want):
        assert np.array_equal(a, b)


def _advance(state, steps):
    for _ in range(steps):
        state = (state * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
    return state


@pytest.mark.parametrize("kvd", KVD, ids=KVD_IDS)
@pytest.mark.parametrize("strategy,slot", [(1, -1), (3, -1), (4, -1), (7, -1), (4, 0)], ids=["std", "top_k", "top_p", "min_p", "top_p-processed"])
def test_full_acceptance_built_token_by_token(kvd, strategy, slot):
    """junk drafts reveal token 0; with it as draft 1 the same call from the same state reveals token 1, and so on: row i depends on
    tokens 0..i only, so the sequence is stable and after n - 1 rounds every draft is accepted"""
    m = _model(kvd)
    n, p, st0 = 6, _params(strategy, 1.1), W.rng_state_of_seed(1234 + strategy)
    if slot >= 0:
        m.arm()
        before = m.state()
    toks = np.concatenate([[m.t0], m.junk[:n - 1]]).astype(np.int32)
    known = 0
    for rounds in range(n):
        out, st = _call(m, toks, p, st0, slot)
        assert len(out) >= known + 1 and [int(t) for t in toks[1:1 + known]] == out[:known]
        assert st == _advance(st0, 2 * len(out))
        if len(out) == n:
            break
        known = len(out)
        toks[1:1 + known] = out[:known]           # (a junk draft that happened to be right only speeds this up)
    assert len(out) == n and [int(t) for t in toks[1:]] == out[:n - 1] and rounds <= n - 1
    if slot >= 0:
        assert np.array_equal(m.state(), before)                       # the call never writes the logit state
        assert 400 not in out                                          # the banned id


@pytest.mark.parametrize("kvd", KVD, ids=KVD_IDS)
def test_greedy_accepts_where_the_greedy_draft_step_agrees(kvd):
    m = _model(kvd)
    n = 6
    toks = np.concatenate([[m.t0], m.junk[:n - 1]]).astype(np.int32)
    ids = m.wk.decode_draft(toks, m.pos0)
    toks[1], toks[2] = ids[0], ids[1]              # two right guesses (row 1 behind the right token 0 may answer differently: recomputed)
    for _ in range(2):
        ids = [int(t) for t in m.wk.decode_draft(toks, m.pos0)]
        e = next((i + 1 for i in range(n - 1) if ids[i] != int(toks[i + 1])), n)
        out, st = _call(m, toks, _params(2, pool=1), 12345)
        assert out == ids[:e] and st == 12345 and e >= 2
        toks[1:e + 1] = ids[:e] if e < n else ids[:n - 1]


def test_the_other_steps_are_not_disturbed():
    m = _model(dt.F16)
    wk, n = m.wk, 5
    toks = np.concatenate([[m.t0], m.junk[:n - 1]]).astype(np.int32)
    p, st0 = _params(), W.rng_state_of_seed(5)
    greedy, _ = wk.decode(m.t0, m.pos0, 6)
    draft = wk.decode_draft(toks, m.pos0)
    sampled, st_s, _ = wk.decode_sampled(m.t0, m.pos0, 6, p, st0)
    m.restore()
    first = _call(m, toks, p, st0)
    assert _call(m, toks, p, st0) == first                               # the replayed step gives the captured one's result
    m.arm()
    _call(m, toks, p, st0, 0)
    m.restore()
    assert np.array_equal(wk.decode(m.t0, m.pos0, 6)[0], greedy)
    assert np.array_equal(wk.decode_draft(toks, m.pos0), draft)
    again, st_a, _ = wk.decode_sampled(m.t0, m.pos0, 6, p, st0)
    assert np.array_equal(again, sampled) and st_a == st_s


def _refused(m, code, word, n=5, pos0=None, p=None, slot=-1, toks=True):
    L = ia.lib()
    p = p or _params()
    st, n_out = C.c_ulonglong(1), C.c_int(0)
    t = np.concatenate([[m.t0], m.junk[:8]]).astype(np.int32)
    out = np.zeros(16, np.int32)
    rc = L.ifa_model_decode_draft_sampled(m.wk._h, n, t.ctypes.data_as(C.c_void_p) if toks else None, m.pos0 if pos0 is None else pos0, C.byref(p),
                                          C.byref(st), slot, out.ctypes.data_as(C.c_void_p), C.byref(n_out))
    assert rc == code and word in L.ifa_last_error() and b"ifa_model_decode_draft_sampled" in L.ifa_last_error(), (rc, L.ifa_last_error())


def test_refusals(tmp_path):
    from inferflow_amd.engine import InferenceEngine
    from tests import engine_fixtures as fx
    m = Model(dt.F16)                              # (a worker of its own: no logit state yet)
    for n, pos0 in ((1, None), (9, None), (0, None)):
        _refused(m, -1, b"rows (2..8", n=n, pos0=pos0)
    for n, pos0 in ((5, MAX_CTX - 4), (2, MAX_CTX - 1), (5, -1)):
        _refused(m, -1, b"outside max_ctx", n=n, pos0=pos0)
    _refused(m, -1, b"null pointer", toks=False)
    _refused(m, -1, b"strategy 10", p=_params(10))                     # mirostat
    _refused(m, -1, b"pool_size 0", p=_params(pool=0))
    _refused(m, -1, b"pool_size 257", p=_params(pool=257))
    _refused(m, -1, b"state slot 0 has no logit state", slot=0)
    _refused(m, -1, b"state slot -2", slot=-2)
    for name in ("exact_order", "perf_stat"):
        m.wk.set_option(name, 1)
        _refused(m, -4, name.encode())
        m.wk.set_option(name, 0)
    for a, b in zip(m.kv(), m.snap):                                   # the refused calls wrote nothing
        assert np.array_equal(a, b)
    # a reached row without a candidate: every id but one excluded leaves pools of one entry; all excluded, an empty pool
    m.wk.set_pool_excluded(list(range(m.V)))
    _refused(m, -4, b"row 0 had no token to draw")
    m.wk.set_pool_excluded([])
    out, _ = m.wk.decode_draft_sampled(np.concatenate([[m.t0], m.junk[:4]]).astype(np.int32), m.pos0, _params(), 1)
    assert 1 <= len(out) <= 5
    m.wk.close()
    for devices, word in (("0&0", b"partitioned"), ("0;0", b"lm_head missing")):
        ini, _ = fx.write_model_dir(str(tmp_path / devices.replace("&", "a").replace(";", "s")), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", maxq=4, devices=devices)
        eng = InferenceEngine.from_ini(ini)
        h = ia.lib().ifa_engine_worker(eng._h, 0)
        assert h
        L = ia.lib()
        p, st, n_out = _params(), C.c_ulonglong(1), C.c_int(0)
        t, out = np.array([5, 6, 7], np.int32), np.zeros(8, np.int32)
        rc = L.ifa_model_decode_draft_sampled(C.c_void_p(h), 3, t.ctypes.data_as(C.c_void_p), 3, C.byref(p), C.byref(st), -1, out.ctypes.data_as(C.c_void_p),
                                              C.byref(n_out))
        assert rc == -4 and word in L.ifa_last_error(), (rc, L.ifa_last_error())
        eng.close()
