"""-m gpu: lookup decoding for seeded sampled and processed queries (`lookup_sampled = true`; InferenceEngine::GenerateLookup ending its
draft steps in ifa_model_decode_draft_sampled).  Exactness: generate_lookup against a reference loop written here and run on a second
engine's worker -- the same kernels on the same bytes, so tokens, LookupStats and the final generator state are equal exactly.  No
comparison with Generate or the Infer / Commit loop: their single-row step rounds differently from the batched rows.  Then the
bookkeeping (limits, context shift, prefix cache), processed queries, and the refusals with the key off."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import _capi
from inferflow_amd import worker as W
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import engine_fixtures as fx
from tests.test_gpu_logit_processors_engine import OPTS, PROMPT

pytestmark = pytest.mark.gpu

CTX, N_NEW = 64, 40
STRATEGY, TEMPERATURE = "sample.top_p", 0.6
# the sampler's defaults (host/sampling_strategy.h: SamplingConfig), which the fixture's model does not override
MAX_K, TOP_P, MIN_P, POOL = 8, 0.9, 0.05, 50
NGRAM_MAX, NGRAM_MIN = 3, 1


def _engine(tmp, ctx=CTX, **keys):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", ctx=ctx)
    keys = dict(dict(device_sampling_pool="true", device_sampler="true", lookup_sampled="true"), **keys)
    extra = "".join("%s = %s\n" % kv for kv in keys.items() if kv[1] is not None)
    text = open(ini).read()
    assert "return_output_tensors = false" in text
    open(ini, "w").write(text.replace("return_output_tensors = false", "return_output_tensors = false\n" + extra))
    return InferenceEngine.from_ini(ini)


class _Borrowed(W.DecodeWorker):
    """the engine's worker under the Python worker's methods; the engine owns it"""

    def __init__(self, eng):
        self._h = C.c_void_p(ia.lib().ifa_engine_worker(eng._h, 0))
        assert self._h

    def close(self):
        pass


def _lookup_draft(ctx, pred, k):
    a = (C.c_int * len(ctx))(*ctx)
    p = (C.c_int * max(1, len(pred)))(*pred) if pred else None
    out = (C.c_int * 8)()
    n = ia.lib().ifa_lookup_draft(a, len(ctx), p, len(pred), NGRAM_MAX, NGRAM_MIN, k, out)
    assert n >= 0
    return [out[i] for i in range(n)]


def _reference(eng, seed, n_new, pred, draft_len, max_ctx=CTX):
    """GenerateLookup's loop restated over the worker of `eng`: the first token and the generator state from generate(q, 1), then
    ifa_lookup_draft with the engine's m_max and decode_sampled (one step) / decode_draft_sampled.  Returns (tokens, stats, state)."""
    q = eng.add_query(PROMPT, strategy=STRATEGY, seed=seed, temperature=TEMPERATURE)
    assert q > 0, eng._err()
    first, _ = eng.generate(q, 1)
    st = eng.query_rng_state(q)
    wk = _Borrowed(eng)
    p = _capi.SampleParams(eng.strategy_id(STRATEGY), TEMPERATURE, TOP_P, MAX_K, MIN_P, POOL)
    tokens, processed, left = list(PROMPT) + first, len(PROMPT), n_new - 1
    stats = dict(steps=1, draft_steps=0, drafted=0, accepted=0)
    while left > 0:
        pos0 = processed
        m_max = min(draft_len, left - 1, max_ctx - pos0 - 1)
        draft = _lookup_draft(tokens, pred, m_max) if m_max >= 1 else []
        stats["steps"] += 1
        if not draft:
            out, st, _ = wk.decode_sampled(tokens[-1], pos0, 1, p, st)
            out = [int(out[0])]
        else:
            out, st = wk.decode_draft_sampled([tokens[-1]] + draft, pos0, p, st)
            out = [int(t) for t in out]
            stats["draft_steps"] += 1
            stats["drafted"] += len(draft)
            stats["accepted"] += len(out) - 1
        tokens += out
        processed = pos0 + len(out)
        left -= len(out)
    assert left == 0
    assert eng.remove_query(q)
    return tokens[len(PROMPT):], stats, st


def _run(eng, seed, n_new, pred, **opts):
    q = eng.add_query(PROMPT, strategy=opts.pop("strategy", STRATEGY), seed=seed, temperature=TEMPERATURE, **opts)
    assert q > 0, eng._err()
    before = eng.model_info("lookup_sampled_steps")
    got, st = eng.generate_lookup(q, n_new, prediction=pred)
    assert eng.model_info("lookup_sampled_steps") - before == st["draft_steps"]
    return q, got, st


@pytest.fixture(scope="module")
def prediction(tmp_path_factory):
    """the tokens of a first run with the same seed: what the second run is expected to repeat"""
    eng = _engine(tmp_path_factory.mktemp("first"))
    assert eng.model_info("lookup_sampled") == 1 and eng.model_info("device_sampler") == 1
    q, got, st = _run(eng, 4321, N_NEW, None)
    eng.close()
    assert len(got) == N_NEW and len(set(got)) > 3
    return got


@pytest.mark.parametrize("draft_len", [1, 4, 7])
@pytest.mark.parametrize("with_prediction", [False, True], ids=["own-tokens", "prediction"])
def test_generate_lookup_equals_the_reference_loop(tmp_path, prediction, draft_len, with_prediction):
    pred = prediction if with_prediction else None
    eng, ref = _engine(tmp_path / "a", lookup_draft_len=draft_len), _engine(tmp_path / "b", lookup_draft_len=draft_len)
    q, got, st = _run(eng, 4321, N_NEW, pred)
    want, want_st, want_state = _reference(ref, 4321, N_NEW, pred or [], draft_len)
    gpu_ms = st.pop("gpu_ms")
    print("draft_len %d %s: %s, acceptance %.2f" % (draft_len, "prediction" if pred else "own tokens", st, st["accepted"] / max(st["drafted"], 1)))
    assert got == want, (got, want)
    assert st == want_st and gpu_ms > 0
    assert eng.query_rng_state(q) == want_state
    assert st["steps"] + st["accepted"] == len(got) == N_NEW
    if with_prediction:
        # the first token comes from the prompt step on both runs, so its 1-gram is found in the prediction: drafts really ran.  (No
        # threshold on the acceptance: the first run's plain steps round differently from the rows of a draft step.)
        assert got[0] == prediction[0] and st["drafted"] > 0
    (qq, tok), = eng.infer()                  # tokens / processed are consistent: the next step runs
    assert qq == q and 0 <= tok < fx.SHAPE["vocab"]
    eng.close()
    ref.close()


def test_limits(tmp_path, prediction):
    eng = _engine(tmp_path, lookup_draft_len=7)
    for n in (1, 2, 5, 10):                   # a prediction far longer than the request: never a token too many
        q, got, st = _run(eng, 4321, n, prediction)
        assert len(got) == n and got[0] == prediction[0] and st["steps"] + st["accepted"] == n, (n, st)
        assert eng.remove_query(q)
    room = CTX - len(PROMPT)
    q = eng.add_query(PROMPT, strategy=STRATEGY, seed=4321, temperature=TEMPERATURE)
    with pytest.raises(EngineError, match="max_context_len"):
        eng.generate_lookup(q, room + 1, prediction=prediction)
    got, st = eng.generate_lookup(q, room, prediction=prediction)      # exactly to the limit
    assert len(got) == room and st["steps"] + st["accepted"] == room and st["drafted"] > 0
    with pytest.raises(EngineError):
        eng.generate_lookup(q, 1)
    eng.close()


def test_across_a_context_shift(tmp_path, prediction):
    n = CTX - len(PROMPT) + 12
    runs = []
    for name in ("a", "b"):
        eng = _engine(tmp_path / name, context_shift="true")
        q, got, st = _run(eng, 4321, n, prediction)
        assert len(got) == n and st["steps"] + st["accepted"] == n and st["drafted"] > 0
        assert eng.model_info("context_shifts") == 1 and eng.query_shifted_tokens(q) > 0
        (qq, tok), = eng.infer()
        assert qq == q
        runs.append((got, st["steps"], st["accepted"], eng.query_rng_state(q)))
        eng.close()
    assert runs[0] == runs[1]


def test_prefix_cache_records_no_rejected_rows(tmp_path, prediction):
    eng = _engine(tmp_path, prefix_cache="true")
    assert eng.model_info("prefix_cache") == 1
    wrong = []
    for t in prediction:                      # every true token followed by a wrong one: the 1-gram matches, its continuation never does
        wrong += [t, t + 1 if t + 1 < fx.SHAPE["vocab"] else 3]
    n = 20
    q, got, st = _run(eng, 4321, n, wrong)
    assert len(got) == n and st["drafted"] > st["accepted"] and st["draft_steps"] > 0, st      # rejected rows really ran
    assert eng.remove_query(q)
    hist = PROMPT + got
    q2 = eng.add_query(hist)
    assert eng.query_cached_tokens(q2) == len(hist) - 1    # the whole processed history and not a row more
    assert eng.prefix_cache_stats() == dict(active=1, hits=1, tokens=len(hist) - 1, copies=0)
    (qq, tok), = eng.infer()
    assert qq == q2 and 0 <= tok < fx.SHAPE["vocab"]
    eng.close()


def _state_row(eng, slot=0):
    V = fx.SHAPE["vocab"]
    wk = _Borrowed(eng)
    return wk.read_buffer("logit_state", nbytes=(slot + 1) * V * 4).view(np.uint32)[slot * V:(slot + 1) * V].copy()


@pytest.mark.parametrize("strategy,seed", [("sample.top_p", 17), ("greedy", 0)])
def test_processed_queries(tmp_path, strategy, seed):
    eng = _engine(tmp_path)
    q, first, _ = _run(eng, seed, 24, None, strategy=strategy, **OPTS)
    assert len(first) == 24 and 400 not in first
    assert eng.remove_query(q)
    q, got, st = _run(eng, seed, 24, first, strategy=strategy, **OPTS)
    print("%s processed: %s" % (strategy, st))
    assert len(got) == 24 and got[0] == first[0] and 400 not in got and st["drafted"] > 0 and st["steps"] + st["accepted"] == 24
    # every committed token counted exactly once, whatever the arithmetic
    counts = np.bincount(np.array(got), minlength=fx.SHAPE["vocab"]).astype(np.uint32)
    assert np.array_equal(_state_row(eng) & np.uint32(0x7FFFFFFF), counts)
    (qq, tok), = eng.infer()
    assert qq == q and tok != 400
    eng.close()


def test_refusals(tmp_path):
    off = _engine(tmp_path / "off", lookup_sampled=None)
    assert off.model_info("lookup_sampled") == 0 and off.model_info("device_sampler") == 1
    q = off.add_query(PROMPT, strategy="sample.top_p", seed=3)
    with pytest.raises(EngineError, match="greedily"):
        off.generate_lookup(q, 4)
    assert off.remove_query(q)
    q = off.add_query(PROMPT, **OPTS)
    with pytest.raises(EngineError, match="logit processors"):
        off.generate_lookup(q, 4)
    off.close()
    nosampler = _engine(tmp_path / "nosampler", device_sampler=None)
    assert nosampler.model_info("lookup_sampled") == 0            # the key alone is inert
    q = nosampler.add_query(PROMPT, strategy="sample.top_p", seed=3)
    with pytest.raises(EngineError, match="greedily"):
        nosampler.generate_lookup(q, 4)
    nosampler.close()
    on = _engine(tmp_path / "on")
    q = on.add_query(PROMPT, strategy="mirostat", seed=3)
    assert q > 0
    with pytest.raises(EngineError, match="mirostat"):
        on.generate_lookup(q, 4)
    assert on.remove_query(q)
    q = on.add_query(PROMPT)                                      # an unprocessed greedy query keeps the greedy draft step
    got, st = on.generate_lookup(q, 8)
    assert len(got) == 8 and on.model_info("lookup_sampled_steps") == 0
    on.close()
