"""-m gpu: sampled and processed queries on the device-fed replay.  Worker level: ifa_model_decode_sampled of 20 steps in one call
against 20 calls of one step, each checked against the pool of the step's own logits row + the draw rule on the host
(ifa_sample_pool_host); the greedy graph before and after; the refusals.  Engine level (`device_sampler = true`): generate() of a
seeded query against the Infer / CommitInferenceResult loop of a second engine, token for token, then four more loop steps on both
(the generator hand-off), the counters, the device penalty state, a Q8 cache, a run across a context shift, the refusals."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import _capi, dtypes as dt, synth
from inferflow_amd import worker as W
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import engine_fixtures as fx
from tests.pool_util import pool_ref
from tests.test_gpu_logit_processors_engine import OPTS, PROMPT

pytestmark = pytest.mark.gpu

STEPS = 20


def _params(strategy=4, temperature=0.9, top_p=0.9, max_k=8, min_p=0.05, pool=50):
    return _capi.SampleParams(strategy, temperature, top_p, max_k, min_p, pool)


def _kv(wk, layers):
    return [wk.read_buffer(n, l).copy() for l in range(layers) for n in ("kcache", "vcache")]


# ------------------------------------------------------------------------------------------------ worker level
@pytest.mark.parametrize("shape,strategy", [("test_gqa", 4), ("test_mha", 7)])
def test_one_call_equals_single_steps_checked_against_the_host_rule(shape, strategy):
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    ok, why = wk.fused_supported()
    assert ok, why
    V = s["vocab"]
    prompt = np.random.default_rng(2).integers(3, V, 6).astype(np.int32)
    tok = wk.forward(prompt, 0)
    pos = len(prompt)
    greedy_before, _ = wk.decode(tok, pos, 8)
    p = _params(strategy)
    st0 = W.rng_state_of_seed(7)
    toks_a, st_a, _ = wk.decode_sampled(tok, pos, STEPS, p, st0)
    kv_a = _kv(wk, s["layers"])
    t, st, toks_b = tok, st0, []
    for i in range(STEPS):
        out, st_new, _ = wk.decode_sampled(t, pos + i, 1, p, st)
        row = wk.read_buffer("logits", nbytes=V * 2).view(np.float16)
        ids, bits = pool_ref(row, 50)
        want_tok, _, _, _, _, want_st = W.sample_pool_host(ids, bits, p, st)
        assert (int(out[0]), st_new) == (want_tok, want_st), (i, int(out[0]), want_tok)
        t, st = int(out[0]), st_new
        toks_b.append(t)
    assert [int(x) for x in toks_a] == toks_b and st_a == st
    assert len(set(toks_b)) > 3                                      # really sampled: not one token over and over
    for a, b in zip(kv_a, _kv(wk, s["layers"])):
        assert np.array_equal(a, b)
    greedy_after, _ = wk.decode(tok, pos, 8)                         # the greedy graph survived the sampled calls
    assert np.array_equal(greedy_before, greedy_after)
    # greedy through the sampled step: the pool's first id, the generator untouched
    out, st_g, _ = wk.decode_sampled(tok, pos, 8, _params(2, pool=1), 12345)
    assert np.array_equal(out, greedy_before) and st_g == 12345
    wk.close()


def test_processors_in_the_sampled_step_count_every_token_once():
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    V = s["vocab"]
    prompt = np.random.default_rng(3).integers(3, V, 6).astype(np.int32)
    tok = wk.forward(prompt, 0)
    pos = len(prompt)
    bias = {int(prompt[0]): 5.0, 17: -100.0, 400: float("-inf")}
    p = _params(4, 1.1)
    st0 = W.rng_state_of_seed(99)

    def reset():
        wk.logit_state_reset(0, prompt, rep=1.3, freq=0.25, pres=0.5, bias=bias)
        wk.logit_state_add([0], [tok])

    reset()
    toks_a, st_a, _ = wk.decode_sampled(tok, pos, STEPS, p, st0, state_slot=0)
    state_a = wk.read_buffer("logit_state", nbytes=V * 4).view(np.uint32).copy()
    reset()
    t, st, toks_b = tok, st0, []
    for i in range(STEPS):
        out, st_new, _ = wk.decode_sampled(t, pos + i, 1, p, st, state_slot=0)
        row = wk.read_buffer("logits_adj", nbytes=V * 2).view(np.float16)
        ids, bits = pool_ref(row, 50)
        want_tok, _, _, _, _, want_st = W.sample_pool_host(ids, bits, p, st)
        assert (int(out[0]), st_new) == (want_tok, want_st), (i, int(out[0]), want_tok)
        t, st = int(out[0]), st_new
        toks_b.append(t)
    assert [int(x) for x in toks_a] == toks_b and st_a == st and 400 not in toks_b
    state_b = wk.read_buffer("logit_state", nbytes=V * 4).view(np.uint32)
    assert np.array_equal(state_a, state_b)
    counts = np.bincount(np.array([tok] + toks_b), minlength=V)
    assert np.array_equal(state_b & np.uint32(0x7FFFFFFF), counts.astype(np.uint32))      # every drawn token exactly once
    wk.close()


def _refused(wk_handle, code, word, p=None, slot=-1):
    L = ia.lib()
    p = p or _params()
    st = C.c_ulonglong(1)
    out = np.zeros(4, np.int32)
    rc = L.ifa_model_decode_sampled(wk_handle, 5, 3, 2, C.byref(p), C.byref(st), slot, out.ctypes.data_as(C.c_void_p), None)
    assert rc == code and word in L.ifa_last_error(), (rc, L.ifa_last_error())


def test_worker_refusals(tmp_path):
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    wk.forward(np.array([5, 6, 7], np.int32), 0)
    for name in ("exact_order", "perf_stat"):
        wk.set_option(name, 1)
        _refused(wk._h, -4, name.encode())
        wk.set_option(name, 0)
    _refused(wk._h, -1, b"strategy", _params(10))                    # mirostat
    _refused(wk._h, -1, b"pool_size", _params(pool=0))
    _refused(wk._h, -1, b"pool_size", _params(pool=257))
    _refused(wk._h, -1, b"state slot", slot=0)                       # no logit state yet
    _refused(wk._h, -1, b"state slot", slot=-2)
    wk.close()
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06, full_quant_gemv=0)
    ok, _ = wk.fused_supported()
    assert not ok
    _refused(wk._h, -4, b"fused decode step does not cover")
    wk.close()
    for devices, word in (("0&0", b"partitioned"), ("0;0", b"lm_head missing")):
        ini, _ = fx.write_model_dir(str(tmp_path / devices.replace("&", "a").replace(";", "s")), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", maxq=4, devices=devices)
        eng = InferenceEngine.from_ini(ini)
        h = ia.lib().ifa_engine_worker(eng._h, 0)
        assert h
        _refused(C.c_void_p(h), -4, word)
        assert eng.model_info("device_sampler") == 0
        eng.close()


# ------------------------------------------------------------------------------------------------ engine level
def _engine(tmp, sampler=True, kvd="F16", ctx=64, shift=False):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd=kvd, ret="false", ctx=ctx)
    keys = "device_sampling_pool = true\n" + ("device_sampler = true\n" if sampler else "") + ("context_shift = true\n" if shift else "")
    text = open(ini).read().replace("return_output_tensors = false", "return_output_tensors = false\n" + keys)
    open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


def _loop(eng, qid, steps):
    toks = []
    for _ in range(steps):
        (q, tok), = eng.infer()
        assert q == qid
        toks.append(tok)
        assert eng.commit({qid: tok})
    return toks


def _state_row(eng, slot=0):
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    p, n = C.c_void_p(), C.c_size_t()
    ia.check(L.ifa_model_get_buffer(C.c_void_p(h), b"logit_state", 0, C.byref(p), C.byref(n)))
    V = fx.SHAPE["vocab"]
    assert p.value and n.value >= (slot + 1) * V * 4
    out = np.empty(V, np.uint32)
    ia.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(p.value + slot * V * 4), out.nbytes, None))
    ia.check(L.ifa_stream_sync(None))
    return out


def _generate_equals_loop(gen, loop, n, strategy, seed, temperature=1.0, **opts):
    qa = gen.add_query(PROMPT, strategy=strategy, seed=seed, temperature=temperature, **opts)
    qb = loop.add_query(PROMPT, strategy=strategy, seed=seed, temperature=temperature, **opts)
    assert qa > 0 and qb > 0, (gen._err(), loop._err())
    before = gen.model_info("device_sampled_steps")
    got, _ = gen.generate(qa, n)
    want = _loop(loop, qb, n)
    assert got == want, (strategy, temperature, got, want)
    assert gen.model_info("device_sampled_steps") - before == n - 1      # the first token is the prompt step's
    assert _loop(gen, qa, 4) == _loop(loop, qb, 4)                      # the generator (and the penalty state) went on where the loop's stands
    if opts:
        assert np.array_equal(_state_row(gen), _state_row(loop))
    more, _ = gen.generate(qa, 3)                                        # and Generate continues behind the loop's steps
    assert more == _loop(loop, qb, 3)
    assert gen.remove_query(qa) and loop.remove_query(qb)
    return got


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    gen = _engine(tmp_path_factory.mktemp("gen"))
    loop = _engine(tmp_path_factory.mktemp("loop"), sampler=False)
    assert gen.model_info("device_sampler") == 1 and loop.model_info("device_sampler") == 0
    yield gen, loop
    gen.close()
    loop.close()


@pytest.mark.parametrize("strategy", ["sample.std", "top_k", "sample.top_p", "min_p"])
@pytest.mark.parametrize("temperature", [0.8, 1.0, 1.3])
def test_generate_equals_the_infer_commit_loop(engines, strategy, temperature):
    got = _generate_equals_loop(engines[0], engines[1], 24, strategy, 4321, temperature)
    assert len(set(got)) > 3


@pytest.mark.parametrize("strategy,seed", [("sample.top_p", 17), ("greedy", 0)])
def test_processed_queries_generate_like_the_loop(engines, strategy, seed):
    got = _generate_equals_loop(engines[0], engines[1], 24, strategy, seed, **OPTS)
    assert 400 not in got                                                # the banned id


def test_with_a_q8_cache(tmp_path):
    gen, loop = _engine(tmp_path / "a", kvd="Q8"), _engine(tmp_path / "b", sampler=False, kvd="Q8")
    _generate_equals_loop(gen, loop, 24, "sample.top_p", 99, 1.0)
    gen.close()
    loop.close()


def test_across_a_context_shift(tmp_path):
    gen, loop = _engine(tmp_path / "a", shift=True), _engine(tmp_path / "b", sampler=False, shift=True)
    qa = gen.add_query(PROMPT, strategy="sample.top_p", seed=5)
    qb = loop.add_query(PROMPT, strategy="sample.top_p", seed=5)
    n = 64 - len(PROMPT) + 12                                            # runs past max_context_len = 64
    got, _ = gen.generate(qa, n)
    assert got == _loop(loop, qb, n)
    assert gen.model_info("context_shifts") == loop.model_info("context_shifts") == 1
    assert gen.query_shifted_tokens(qa) == loop.query_shifted_tokens(qb) > 0
    gen.close()
    loop.close()


def test_engine_refusals(tmp_path, engines):
    off = _engine(tmp_path, sampler=False)
    q = off.add_query(PROMPT, strategy="sample.top_p", seed=3)
    with pytest.raises(EngineError, match="greedily"):
        off.generate(q, 4)
    assert off.remove_query(q)
    q = off.add_query(PROMPT, **OPTS)
    with pytest.raises(EngineError, match="logit processors"):
        off.generate(q, 4)
    off.close()
    gen = engines[0]
    q = gen.add_query(PROMPT, strategy="mirostat", seed=3)
    assert q > 0
    with pytest.raises(EngineError, match="mirostat"):
        gen.generate(q, 4)
    assert gen.remove_query(q)
    q = gen.add_query(PROMPT, strategy="sample.top_p", seed=3)
    with pytest.raises(EngineError, match="greedily"):                   # lookup decoding stays greedy
        gen.generate_lookup(q, 4)
    assert gen.remove_query(q)
