"""-m gpu: the prompt prefix cache through the InferenceEngine (`prefix_cache = true`): a hit on a busy slot goes through the device
copy and computes what the original rows compute, a hit on a free slot is taken in place, the cap, the threshold, record hygiene
after score(), and the engines on which the key changes nothing (key off; return_output_tensors = true)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd.engine import InferenceEngine
from tests import engine_fixtures as fx
from tests import gpu_util as g

pytestmark = pytest.mark.gpu

V, LAYERS, CTX = fx.SHAPE["vocab"], fx.SHAPE["layers"], 128
RNG = np.random.default_rng(23)
S = [int(t) for t in RNG.integers(3, V, 40)]


def _more(n, first_not=None):
    while True:
        t = [int(x) for x in RNG.integers(3, V, n)]
        if first_not is None or t[0] != first_not:
            return t


def _engines(tmp, ret="false"):
    """(ini with prefix_cache = true, ini without the key) over ONE model directory"""
    off, _ = fx.write_model_dir(str(tmp), ret=ret, maxq=4, ctx=CTX)
    text = open(off).read()
    assert "dynamic_batching_min_queries = 2\n" in text
    on = str(tmp / "engine_on.ini")
    open(on, "w").write(text.replace("dynamic_batching_min_queries = 2\n", "dynamic_batching_min_queries = 2\nprefix_cache = true\n"))
    return on, off


def _slot(eng, slot):
    """[layer] -> (K bytes, V bytes) of a slot, read through the engine's worker"""
    L = ia.lib()
    h = C.c_void_p(L.ifa_engine_worker(eng._h, 0))
    ia.check(L.ifa_model_select_kv(h, slot))
    out = []
    for l in range(LAYERS):
        pair = []
        for name in (b"kcache", b"vcache"):
            p, n = C.c_void_p(), C.c_size_t()
            ia.check(L.ifa_model_get_buffer(h, name, l, C.byref(p), C.byref(n)))
            a = np.empty(n.value, np.uint8)
            ia.check(L.ifa_memcpy_d2h(a.ctypes.data_as(C.c_void_p), p, n.value, None))
            ia.check(L.ifa_stream_sync(None))
            pair.append(a)
        out.append(tuple(pair))
    return out


def _row_bytes(eng):
    return _slot(eng, 0)[0][0].size // CTX


def _step(eng, qid):
    res = dict(eng.infer())
    assert qid in res, res
    return res[qid]


def test_hit_on_a_busy_slot_goes_through_the_copy(tmp_path):
    on, _ = _engines(tmp_path)
    eng = InferenceEngine.from_ini(on)
    assert eng.model_info("prefix_cache") == 1 and eng.prefix_cache_stats() == dict(active=1, hits=0, tokens=0, copies=0)
    a_tail = _more(5)
    b_tail = _more(7, first_not=a_tail[0])
    qa = eng.add_query(S + a_tail)
    assert qa > 0, eng._err()
    _step(eng, qa)                                   # A stays active: its slot is busy
    qb = eng.add_query(S + b_tail, logprobs=20)
    assert qb > 0, eng._err()
    assert eng.query_cached_tokens(qb) == 40 and eng.query_cached_tokens(qa) == 0 and eng.query_cached_tokens(qb + 100) == -1
    assert eng.prefix_cache_stats() == dict(active=1, hits=1, tokens=40, copies=1)
    tok_b = _step(eng, qb)
    _, top = eng.last_logprobs(qb)
    assert len(top) == 20
    rb = _row_bytes(eng)
    sa, sb = _slot(eng, 0), _slot(eng, 1)            # A took the lowest slot, B the next one with an empty record
    for l in range(LAYERS):
        for kv in (0, 1):
            assert sa[l][kv][:40 * rb].any()
            assert np.array_equal(sb[l][kv][:40 * rb], sa[l][kv][:40 * rb]), (l, kv)
            assert not np.array_equal(sb[l][kv][40 * rb:47 * rb], sa[l][kv][40 * rb:47 * rb])      # (their own tails)
    assert eng.remove_query(qa) and eng.remove_query(qb)
    # the ORIGINAL rows give the same step: B's tail behind A's slot's 40 rows, through the worker
    L = ia.lib()
    h = C.c_void_p(L.ifa_engine_worker(eng._h, 0))
    ia.check(L.ifa_model_select_kv(h, 0))
    lg = torch.empty((7, V), dtype=torch.float16, device="cuda")
    toks = np.asarray(b_tail, np.int32)
    nxt = C.c_int(-1)
    ia.check(L.ifa_model_forward(h, toks.ctypes.data_as(C.c_void_p), 7, 40, C.c_void_p(lg.data_ptr()), C.byref(nxt)))
    assert nxt.value == tok_b
    row = g.host(lg).astype(np.float32)[-1]
    row[0] = -np.inf                                 # (the unk id is never offered: SortedTopK)
    assert int(np.argmax(row)) == tok_b
    order = sorted(range(V), key=lambda i: (-row[i], i))[:20]
    assert [i for i, _ in top] == order
    eng.close()


def test_hit_on_a_free_slot_is_taken_in_place_and_the_cap(tmp_path):
    on, _ = _engines(tmp_path)
    eng = InferenceEngine.from_ini(on)
    c_prompt = S + _more(5)
    qc = eng.add_query(c_prompt)
    hist = list(c_prompt)
    for _ in range(3):
        t = _step(eng, qc)
        assert eng.commit({qc: t})
        hist.append(t)
    processed = len(hist) - 1                        # 45 prompt tokens + 3 committed; the last one has not run
    other = eng.add_query(_more(30))                 # a bystander in the next slot
    assert other > 0
    _step(eng, other)
    assert eng.remove_query(qc)
    copies = eng.model_info("prefix_cache_copies")
    rb = _row_bytes(eng)
    before0, before2 = _slot(eng, 0), _slot(eng, 2)
    d_prompt = hist[:processed] + _more(3)
    qd = eng.add_query(d_prompt)
    assert qd > 0, eng._err()
    assert eng.query_cached_tokens(qd) == processed == 47
    assert eng.model_info("prefix_cache_copies") == copies == 0 and eng.model_info("prefix_cache_hits") == 1
    _step(eng, qd)
    after0, after2 = _slot(eng, 0), _slot(eng, 2)
    for l in range(LAYERS):
        for kv in (0, 1):                            # D ran in C's old slot 0: its new rows are there, slot 2 was not touched
            assert np.array_equal(after0[l][kv][:processed * rb], before0[l][kv][:processed * rb])
            assert not np.array_equal(after0[l][kv][processed * rb:50 * rb], before0[l][kv][processed * rb:50 * rb])
            assert np.array_equal(after2[l][kv], before2[l][kv])
    # the cap: a prompt EQUAL to a record reuses all but one row and still yields a token
    assert eng.remove_query(qd)                      # record: all 50 tokens of D
    qe = eng.add_query(d_prompt)
    assert qe > 0 and eng.query_cached_tokens(qe) == len(d_prompt) - 1
    t = _step(eng, qe)
    assert 0 < t < V
    assert eng.commit({qe: t})
    assert 0 < _step(eng, qe) < V
    eng.close()


def test_threshold_and_record_hygiene_after_score(tmp_path):
    on, _ = _engines(tmp_path)
    eng = InferenceEngine.from_ini(on)
    qx = eng.add_query(S + _more(4))
    _step(eng, qx)
    assert eng.remove_query(qx)                      # slot 0 now records S + 4
    # an 8-token common prefix is below prefix_cache_min_tokens = 16
    q8 = eng.add_query(S[:8] + _more(20, first_not=S[8]))
    assert q8 > 0 and eng.query_cached_tokens(q8) == 0 and eng.model_info("prefix_cache_hits") == 0
    assert eng.remove_query(q8)                      # (never ran: it leaves an empty record in ITS slot, slot 1)
    # the record is there ...
    qy = eng.add_query(S + _more(6))
    assert eng.query_cached_tokens(qy) == 40 and eng.model_info("prefix_cache_hits") == 1
    assert eng.remove_query(qy)                      # (never ran: slot 0 keeps the 40 rows it matched)
    # ... until score() takes the lowest free slot for its own prompt
    lp = eng.score(_more(24))
    assert lp.shape == (23,) and np.isfinite(lp).all()
    qz = eng.add_query(S + _more(6))
    assert qz > 0 and eng.query_cached_tokens(qz) == 0, "a record survived score() overwriting its slot"
    assert eng.model_info("prefix_cache_hits") == 1 and eng.model_info("prefix_cache_tokens") == 40
    assert 0 < _step(eng, qz) < V
    eng.close()


def test_key_off_changes_nothing(tmp_path):
    _, off = _engines(tmp_path)
    eng = InferenceEngine.from_ini(off)
    assert eng.prefix_cache_stats() == dict(active=0, hits=0, tokens=0, copies=0)
    q1, q2 = eng.add_query(S + _more(5)), eng.add_query(S + _more(5))
    assert q1 > 0 and q2 > 0 and eng.query_cached_tokens(q1) == 0 and eng.query_cached_tokens(q2) == 0
    res = dict(eng.infer())
    assert set(res) == {q1, q2}
    assert eng.remove_query(q1)
    before = [_slot(eng, s) for s in range(3)]
    q3 = eng.add_query(S + _more(9))                 # S is in both slots: still prefilled from row 0, in the lowest free slot
    assert q3 > 0 and eng.query_cached_tokens(q3) == 0
    _step(eng, q3)
    after = [_slot(eng, s) for s in range(3)]
    rb = _row_bytes(eng)
    for l in range(LAYERS):
        for kv in (0, 1):
            assert not np.array_equal(after[0][l][kv][40 * rb:49 * rb], before[0][l][kv][40 * rb:49 * rb])
            assert np.array_equal(after[1][l][kv], before[1][l][kv]) and np.array_equal(after[2][l][kv], before[2][l][kv])
    assert eng.prefix_cache_stats() == dict(active=0, hits=0, tokens=0, copies=0)
    eng.close()


def test_output_tensor_engines_keep_every_row(tmp_path):
    on, _ = _engines(tmp_path, ret="true")
    eng = InferenceEngine.from_ini(on)
    assert eng.model_info("prefix_cache") == 0
    prompt = S + _more(5)
    for _ in range(2):
        q = eng.add_query(prompt)
        assert q > 0 and eng.query_cached_tokens(q) == 0
        _step(eng, q)
        assert eng.last_logits(q).shape == (len(prompt), V)
        assert eng.remove_query(q)
    assert eng.prefix_cache_stats() == dict(active=0, hits=0, tokens=0, copies=0)
    eng.close()


def test_min_tokens_key_is_validated(tmp_path):
    on, _ = _engines(tmp_path)
    bad = str(tmp_path / "engine_bad.ini")
    open(bad, "w").write(open(on).read().replace("prefix_cache = true\n", "prefix_cache = true\nprefix_cache_min_tokens = 0\n"))
    with pytest.raises(Exception, match="prefix_cache_min_tokens"):
        InferenceEngine.from_ini(bad)
