"""-m gpu: steps that end in a device-built candidate pool -- the worker entry points (decode_pool / decode_batch_pool /
forward_pool) against SortedTopK of the step's own logits, and the InferenceEngine with device_sampling_pool = true against
the oracle sampler applied to the worker's logits row of every step."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth
from inferflow_amd.engine import InferenceEngine
from oracle import sampling as S
from tests import engine_fixtures as fx
from tests.pool_util import pool_ref

pytestmark = pytest.mark.gpu


def _check_pool(row_bits, ids, bits, k, excluded=()):
    row = np.ascontiguousarray(row_bits).view(np.float16)
    want_ids, want_bits = pool_ref(row, k, excluded)
    assert np.array_equal(ids, want_ids) and np.array_equal(bits, want_bits)
    if not len(excluded) and not np.isnan(row.astype(np.float32)).any():
        want = S.sorted_top_k(row, k)                           # the oracle's own statement of the pool
        assert [int(i) for i in ids] == [i for i, _ in want]
        assert [float(v) for v in bits.view(np.float16)] == [v for _, v in want]


# ------------------------------------------------------------------------------------------------ worker level
def test_decode_pool_equals_sorted_top_k_of_the_steps_logits():
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    ok, why = wk.fused_supported()
    assert ok, why
    V = s["vocab"]
    prompt = np.random.default_rng(2).integers(3, V, 6).astype(np.int32)
    tok, ids, bits = wk.forward_pool(prompt, 0, 50)             # the prompt step: pool of the LAST row
    rows = wk.read_buffer("logits", nbytes=len(prompt) * V * 2).view(np.uint16).reshape(len(prompt), V)
    _check_pool(rows[-1], ids, bits, 50)
    assert tok == int(ids[0])
    import torch
    lg = torch.zeros((len(prompt), V), dtype=torch.float16, device="cuda")
    wk.reset()
    tok2, ids2, bits2 = wk.forward_pool(prompt, 0, 50, lg)      # with the logits of every row kept: the pool of exactly that last row
    _check_pool(lg[-1].cpu().numpy().view(np.uint16), ids2, bits2, 50)
    assert tok2 == int(ids2[0])
    pos = len(prompt)
    for step in range(20):
        nxt, ids, bits = wk.decode_pool(tok, pos, 50)
        row = wk.read_buffer("logits").view(np.uint16)
        assert ids.size == 50
        _check_pool(row, ids, bits, 50)
        assert nxt == int(ids[0])                               # nothing excluded: the greedy id leads the pool
        ref, _ = wk.decode(tok, pos, 1)                         # the plain step on the same cache rows: same id
        assert int(ref[0]) == nxt
        tok, pos = nxt, pos + 1
    # a mask of any length (the greedy argmax stops at 3 ids)
    excl = [int(i) for i in ids[:7]]
    wk.set_pool_excluded(excl)
    nxt, ids2, bits2 = wk.decode_pool(tok, pos, 8)
    _check_pool(wk.read_buffer("logits").view(np.uint16), ids2, bits2, 8, excl)
    assert not set(excl) & set(int(i) for i in ids2)
    wk.set_pool_excluded([])
    # the other routes of ifa_model_decode end in the same pool: op-by-op (fused = 0) and the order-exact step
    for opt in ("fused", "exact_order"):
        wk.set_option(opt, 0 if opt == "fused" else 1)
        nxt, ids3, bits3 = wk.decode_pool(tok, pos, 50)
        _check_pool(wk.read_buffer("logits").view(np.uint16), ids3, bits3, 50)
        assert nxt == int(ids3[0])
        wk.set_option(opt, 1 if opt == "fused" else 0)
    L = ia.lib()
    buf = np.zeros(512, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.ifa_model_decode_pool(wk._h, tok, pos, 0, None, p, p, p) == -1 and L.ifa_model_decode_pool(wk._h, tok, pos, 257, None, p, p, p) == -1
    wk.close()


def test_decode_batch_pool_over_three_kv_slots_with_ragged_activity():
    wk, _, s = synth.build("test_mha", dt.Q4_B32T1A, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)      # vocab 777: odd row starts
    V = s["vocab"]
    wk.kv_slots(3)
    rng = np.random.default_rng(3)
    cur = [int(t) for t in rng.integers(0, V, 3)]
    pos = [0, 0, 0]
    for step in range(12):
        act = [0, 1, 2] if step % 3 else [2, 0]                 # (ragged: not every query advances in every step)
        sel = list(range(len(act))) if step % 2 else [len(act) - 1]
        nxt, pools = wk.decode_batch_pool([cur[q] for q in act], [pos[q] for q in act], act, 50, sel)
        rows = wk.read_buffer("logits", nbytes=len(act) * V * 2).view(np.uint16).reshape(len(act), V)
        assert len(pools) == len(sel)
        for j, r in enumerate(sel):
            ids, bits = pools[j]
            _check_pool(rows[r], ids, bits, 50)
            assert int(nxt[r]) == int(ids[0])
        for j, q in enumerate(act):
            assert int(nxt[j]) == int(np.argmax(rows[j].view(np.float16).astype(np.float32)))
            cur[q], pos[q] = int(nxt[j]), pos[q] + 1
    wk.set_option("exact_order", 1)
    L = ia.lib()
    a = np.zeros(256, np.int32); p = a.ctypes.data_as(C.c_void_p)
    z = np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)
    assert L.ifa_model_decode_batch_pool(wk._h, 1, z, z, z, p, 8, z, 1, p, p, p) == -4 and b"exact_order" in L.ifa_last_error()      # IFA_ERR_STATE
    wk.close()


# ------------------------------------------------------------------------------------------------ engine level
def _engine(tmp, pool_key, invalid=None, maxq=6):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", maxq=maxq)
    if pool_key is not None:
        text = open(ini).read().replace("return_output_tensors = false", "return_output_tensors = false\ndevice_sampling_pool = %s" % pool_key)
        assert "device_sampling_pool" in text
        open(ini, "w").write(text)
    if invalid:
        path = os.path.join(str(tmp), "model_spec.json")
        spec = json.load(open(path)); spec["invalid_token_ids"] = [int(i) for i in invalid]
        json.dump(spec, open(path, "w"))
    return InferenceEngine.from_ini(ini)


def _tap(eng, n_rows, V):
    """the worker's logits rows of the step that just ran ([n_rows][V] F16)"""
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    assert h
    p, n = C.c_void_p(), C.c_size_t()
    ia.check(L.ifa_model_get_buffer(C.c_void_p(h), b"logits", 0, C.byref(p), C.byref(n)))
    out = np.empty(n_rows * V, np.float16)
    ia.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, None))
    ia.check(L.ifa_stream_sync(None))
    return out.reshape(n_rows, V)


def _offered(row, excluded=(0,)):
    """the row as the sampler sees it: the excluded ids (the engine's unk id 0) can never enter a pool"""
    r = row.copy()
    r[list(excluded)] = np.float16("-inf")
    return r


PROMPT = [int(t) for t in np.random.default_rng(5).integers(3, 1000, 7)]
STD_FAMILY = {"sample.top_p": S.TOP_P, "sample.std": S.STD, "top_k": S.TOP_K}
EX_FAMILY = {"min_p": S.MIN_P, "tfs": S.TFS, "typical": S.TYPICAL, "mirostat": S.MIROSTAT}


def _run(eng, strategy, seed, temperature, steps, check=True):
    """one seeded query, `steps` tokens; every token against the oracle sampler on the worker's logits row of that step"""
    V = 1000
    qid = eng.add_query(PROMPT, strategy=strategy, seed=seed, temperature=temperature)
    assert qid > 0
    rng, toks, mu, st = S.JavaRandom(seed), [], None, S.FsdState()
    text = list(PROMPT)
    for step in range(steps):
        (q, tok), = eng.infer()
        if check:
            n_rows = len(PROMPT) if step == 0 else 1
            row = _offered(_tap(eng, n_rows, V)[-1])
            if strategy in STD_FAMILY:
                (want, _), _ = S.choose_tokens(row, STD_FAMILY[strategy], rng, temperature=temperature)
            elif strategy in EX_FAMILY:
                (want, _), _, mu = S.choose_tokens_ex(row, EX_FAMILY[strategy], rng, temperature=temperature, mu=mu)
            else:
                (want, _), _ = S.choose_tokens_fsd(row, S.FSD if strategy == "fsd" else S.RANDOM_FSD, rng, st, text, temperature=temperature)
            assert tok == want, (strategy, step)
        toks.append(tok)
        assert eng.commit({qid: tok})
    assert eng.remove_query(qid)
    return toks


def test_engine_sampled_queries_on_the_pool_route(tmp_path):
    eng = _engine(tmp_path / "on", "true")
    assert eng.model_info("device_sampling_pool") == 1 and eng.model_info("sampled_fused_steps") == 0
    L = ia.lib()
    why = C.create_string_buffer(256)
    assert L.ifa_model_fused_supported(C.c_void_p(L.ifa_engine_worker(eng._h, 0)), why, 256) == 1, why.value
    texts = {}
    for i, name in enumerate(list(STD_FAMILY) + list(EX_FAMILY)):
        before = eng.model_info("sampled_fused_steps")
        texts[name] = _run(eng, name, 11 + i, [1.0, 1.3, 0.8][i % 3], steps=8)
        # route proof: the 7 single-token steps took the worker's decode step + pool, none ifa_model_forward + a logits row
        assert eng.model_info("sampled_fused_steps") == before + 7, name
    assert _run(eng, "sample.top_p", 11, 1.0, steps=8, check=False) == texts["sample.top_p"]        # same seed, same text
    assert len({tuple(t) for t in texts.values()}) >= 4
    for name in ("fsd", "random_fsd"):
        _run(eng, name, 31, 1.0, steps=12)
    # a batched step: two sampled queries and a greedy one advance together; each row's id from its own logits row
    before = eng.model_info("sampled_fused_steps")
    q1 = eng.add_query(PROMPT, strategy="sample.std", seed=21, temperature=1.5)
    q2 = eng.add_query(PROMPT[:5])
    q3 = eng.add_query(PROMPT[:6], strategy="top_k", seed=23)
    order = sorted([q1, q2, q3])
    rngs = {q1: (S.JavaRandom(21), S.STD, 1.5), q3: (S.JavaRandom(23), S.TOP_K, 1.0)}
    res = dict(eng.infer())                                      # the three prompt steps, one by one
    assert set(res) == {q1, q2, q3}
    for q, (rng, sid, temp) in rngs.items():                     # (their rows were overwritten by the later prompts: replay the draw only)
        rng.next(26); rng.next(27)
    assert eng.commit(res)
    for _ in range(5):
        res = dict(eng.infer())
        assert set(res) == {q1, q2, q3}
        rows = _tap(eng, 3, 1000)
        for q, (rng, sid, temp) in rngs.items():
            (want, _), _ = S.choose_tokens(_offered(rows[order.index(q)]), sid, rng, temperature=temp)
            assert res[q] == want
        assert res[q2] == int(np.argmax(_offered(rows[order.index(q2)]).astype(np.float32)))
        assert eng.commit(res)
    assert eng.model_info("sampled_fused_steps") == before + 10   # two sampled rows in each of five batched steps
    for q in (q1, q2, q3):
        assert eng.remove_query(q)
    eng.close()
    # key off / absent: the host path draws the same tokens on this small llama-style model (fused step == op-by-op step here)
    for sub, key in (("off", "false"), ("absent", None)):
        e2 = _engine(tmp_path / sub, key)
        assert e2.model_info("device_sampling_pool") == 0
        for i, name in enumerate(list(STD_FAMILY) + list(EX_FAMILY)):
            assert _run(e2, name, 11 + i, [1.0, 1.3, 0.8][i % 3], steps=8, check=False) == texts[name], (sub, name)
        assert e2.model_info("sampled_fused_steps") == 0
        e2.close()


def test_engine_greedy_over_a_vocabulary_with_five_excluded_ids(tmp_path):
    """more excluded ids than the device argmax holds (3): greedy queries take the pool route with k = 1"""
    e0 = _engine(tmp_path / "plain", "true")
    q = e0.add_query(PROMPT)
    seen = []
    for _ in range(8):
        (qq, tok), = e0.infer()
        seen.append(tok); e0.commit({q: tok})
    e0.close()
    invalid = sorted(set(seen))[:4]
    assert len(invalid) == 4 and 0 not in invalid
    excluded = [0] + invalid                                     # the unk id + four Invalid-type tokens
    eng = _engine(tmp_path / "masked", "true", invalid=invalid)
    q = eng.add_query(PROMPT)
    for step in range(8):
        (qq, tok), = eng.infer()
        row = _offered(_tap(eng, len(PROMPT) if step == 0 else 1, 1000)[-1], excluded)
        assert tok == int(np.argmax(row.astype(np.float32))) and tok not in excluded
        assert eng.commit({q: tok})
    assert eng.model_info("sampled_fused_steps") == 7
    # two such queries share batched steps
    q2 = eng.add_query(PROMPT[:4])
    res = dict(eng.infer())
    assert eng.commit(res)
    order = sorted([q, q2])
    for _ in range(3):
        res = dict(eng.infer())
        rows = _tap(eng, 2, 1000)
        for qq in (q, q2):
            assert res[qq] == int(np.argmax(_offered(rows[order.index(qq)], excluded).astype(np.float32))) and res[qq] not in excluded
        assert eng.commit(res)
    eng.close()
