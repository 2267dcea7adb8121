"""-m gpu: lookup decoding through the InferenceEngine (GenerateLookup / ifa_engine_generate_lookup): the tokens equal the CPU
oracle's greedy sequence whatever the drafts are -- none, all right, all wrong --, the step counts show the drafts being used, the
query's bookkeeping (tokens / processed) stays consistent, max_new_tokens and max_context_len are exact limits, the prefix cache
never records a rejected row, and the engines without the feature refuse the call."""
import math

import numpy as np
import pytest

from inferflow_amd import dtypes as dt
from inferflow_amd.engine import InferenceEngine, EngineError
from tests import engine_fixtures as fx
from tests.model_util import oracle_model_from_host

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.03          # tests/test_gpu_engine.py
V, CTX, N_PROMPT, N_NEW = fx.SHAPE["vocab"], 128, 12, 48
SEED = 801                # see test_oracle_precondition
PROMPT = [int(t) for t in np.random.default_rng(SEED).integers(3, V, N_PROMPT)]

_STATE = {}


def _oracle_run():
    """(ids, top-2 gaps): the oracle's greedy tokens behind PROMPT -- the prompt row and N_NEW single steps -- in the arithmetic of
    the batched rows (F16 activations: full_quant_gemv = 0); _STATE also keeps the same run with the single row's int8-activation
    products (full_quant_gemv = 1, what Generate and a plain step compute).  Computed once."""
    if "ids" not in _STATE:
        w = fx.make_weights(fx.SHAPE, 5, 0.06)
        host = fx.host_tensors(w, fx.SHAPE, dt.Q4_B32T1A)
        for fq in (0, 1):
            om = oracle_model_from_host(host, fx.SHAPE, CTX, dt.Q8_B32T2, rope_order=1, unk_id=0, full_quant_gemv=fq)
            tok, lg = om.forward(np.asarray(PROMPT, np.int32), 0, nthreads=8)
            rows, ids = [lg[-1]], [int(tok)]
            for i in range(N_NEW):
                tok, lg = om.forward(np.array([tok], np.int32), N_PROMPT + i, nthreads=8)
                rows.append(lg[0]); ids.append(int(tok))
            gaps = [float(r[-1] - r[-2]) for r in (np.sort(np.asarray(x, np.float32)) for x in rows)]
            _STATE["ids" if fq == 0 else "ids8"], _STATE["gaps" if fq == 0 else "gaps8"] = ids, gaps
    return _STATE["ids"], _STATE["gaps"]


def _ini(tmp, ret="false", **keys):
    """an engine .ini over ONE model directory per test (llama2.c checkpoint, Q4 weights, Q8 cache), with extra engine keys"""
    base, _ = fx.write_model_dir(str(tmp), ret=ret, maxq=4, ctx=CTX)
    text = open(base).read()
    assert "dynamic_batching_min_queries = 2\n" in text
    extra = "".join("%s = %s\n" % kv for kv in keys.items())
    path = str(tmp / ("engine_%s.ini" % "_".join("%s%s" % kv for kv in keys.items()) if keys else "engine_plain.ini"))
    open(path, "w").write(text.replace("dynamic_batching_min_queries = 2\n", "dynamic_batching_min_queries = 2\n" + extra))
    return path


def _shifted(ids):
    return [t + 1 if t + 1 < V else 3 for t in ids]


def _all_wrong(ids):
    """every true token followed by a wrong one: the 1-gram key always matches, its continuation never does"""
    sh, out = _shifted(ids), []
    for i in range(len(ids) - 1):
        out += [ids[i], sh[i + 1]]
    return out


def test_oracle_precondition():
    """SEED 801: the oracle's prompt row and all 48 steps (49 rows) have a top-2 gap above LOGIT_TOL; the smallest is 0.033203125.
    The seed was picked with the oracle alone, among prompt seeds 0..3000, as the first that also meets two conditions without
    which the assertions below say nothing about the engine:
      * the 48 tokens hold no n-gram (n <= 3) that occurs twice with two different continuations -- with such a repeat (seed 0
        clears the bound with 0.046875 but runs 219 219 219 219 925) the lookup rule itself, lowest start first, drafts a wrong token
        out of a correct prediction, or a right one out of the context under a wrong prediction;
      * the oracle with the single row's int8-activation products (what Generate and a plain step compute) gives the same 49 ids,
        every gap above LOGIT_TOL again (smallest 0.03515625) -- seed 2591 meets everything else with 0.03125, and the two oracles
        part at its step 43, where the int8 run's gap is 0: the device's plain step chose exactly the int8 oracle's token there."""
    ids, gaps = _oracle_run()
    print("oracle: min top-2 gap %.6f over %d rows; int8-activation oracle %.6f" % (min(gaps), len(gaps), min(_STATE["gaps8"])))
    assert len(gaps) == N_NEW + 1 and min(gaps) > LOGIT_TOL, (min(gaps), int(np.argmin(gaps)))
    assert _STATE["ids8"] == ids and min(_STATE["gaps8"]) > LOGIT_TOL, min(_STATE["gaps8"])


def test_plain_and_lookup_without_prediction_equal_the_oracle(tmp_path):
    ids, _ = _oracle_run()
    eng = InferenceEngine.from_ini(_ini(tmp_path))
    assert eng.model_info("lookup_decoding") == 1
    q = eng.add_query(PROMPT)
    plain, _ = eng.generate(q, N_NEW)
    assert plain == ids[:N_NEW]
    assert eng.remove_query(q)
    q = eng.add_query(PROMPT)
    got, st = eng.generate_lookup(q, N_NEW)
    assert got == ids[:N_NEW], st
    assert st["steps"] <= N_NEW and st["draft_steps"] <= st["steps"] and 0 <= st["accepted"] <= st["drafted"] and st["gpu_ms"] > 0
    assert st["steps"] + st["accepted"] == N_NEW           # every step yields one token, every accepted draft one more
    (qq, tok), = eng.infer()                                # processed / tokens are consistent: the next step continues the sequence
    assert qq == q and tok == ids[N_NEW]
    assert eng.generate_lookup(q, 0) == ([], dict(steps=0, draft_steps=0, drafted=0, accepted=0, gpu_ms=0.0))
    eng.close()


@pytest.mark.parametrize("draft_len", [1, 4, 7])
def test_fully_correct_prediction(tmp_path, draft_len):
    ids, _ = _oracle_run()
    eng = InferenceEngine.from_ini(_ini(tmp_path, lookup_draft_len=draft_len))
    q = eng.add_query(PROMPT)
    got, st = eng.generate_lookup(q, N_NEW, prediction=ids[:N_NEW])
    print("draft_len %d: %s" % (draft_len, st))
    assert got == ids[:N_NEW], st
    assert st["accepted"] == st["drafted"] and st["drafted"] > 0, st
    assert st["steps"] <= math.ceil(N_NEW / (draft_len + 1)) + 2, st
    assert st["steps"] + st["accepted"] == N_NEW
    (qq, tok), = eng.infer()
    assert qq == q and tok == ids[N_NEW]
    assert eng.commit({q: tok})
    (qq, tok2), = eng.infer()                               # and one more step behind the committed token runs (no oracle row for it)
    assert qq == q and 0 <= tok2 < V
    eng.close()


@pytest.mark.parametrize("kind", ["ids-shifted-by-one", "wrong-continuations"])
def test_fully_wrong_prediction(tmp_path, kind):
    ids, _ = _oracle_run()
    eng = InferenceEngine.from_ini(_ini(tmp_path))
    q = eng.add_query(PROMPT)
    pred = _shifted(ids[:N_NEW]) if kind == "ids-shifted-by-one" else _all_wrong(ids[:N_NEW])
    got, st = eng.generate_lookup(q, N_NEW, prediction=pred)
    print("%s: %s" % (kind, st))
    assert got == ids[:N_NEW], st
    assert st["accepted"] == 0, st
    if kind == "wrong-continuations":
        assert st["draft_steps"] >= N_NEW // 2 and st["drafted"] > st["draft_steps"], st      # the rejected rows really ran
    assert st["steps"] == N_NEW
    (qq, tok), = eng.infer()
    assert qq == q and tok == ids[N_NEW]
    eng.close()


def test_max_new_tokens_and_the_context_limit(tmp_path):
    ids, _ = _oracle_run()
    eng = InferenceEngine.from_ini(_ini(tmp_path, lookup_draft_len=7))
    for n in (1, 2, 5, 10):                                # a prediction far longer than the request: never a token too many
        q = eng.add_query(PROMPT)
        got, st = eng.generate_lookup(q, n, prediction=ids[:N_NEW])
        assert got == ids[:n], (n, st)
        assert eng.remove_query(q)
    q = eng.add_query(PROMPT)
    room = CTX - N_PROMPT
    with pytest.raises(EngineError, match="max_context_len"):
        eng.generate_lookup(q, room + 1, prediction=ids[:N_NEW])
    got, st = eng.generate_lookup(q, room, prediction=ids[:N_NEW])     # exactly to the limit
    assert len(got) == room and got[:N_NEW] == ids[:N_NEW], st
    assert st["steps"] + st["accepted"] == room
    with pytest.raises(EngineError):
        eng.generate_lookup(q, 1)
    eng.close()


def test_prefix_cache_records_no_rejected_rows(tmp_path):
    ids, _ = _oracle_run()
    eng = InferenceEngine.from_ini(_ini(tmp_path, prefix_cache="true"))
    assert eng.model_info("prefix_cache") == 1 and eng.model_info("lookup_decoding") == 1
    n = 20
    q = eng.add_query(PROMPT)
    got, st = eng.generate_lookup(q, n, prediction=_all_wrong(ids[:N_NEW]))
    assert got == ids[:n] and st["accepted"] == 0 and st["drafted"] > st["draft_steps"] > 0, st
    assert eng.remove_query(q)
    hist = PROMPT + got
    q2 = eng.add_query(hist)
    assert eng.query_cached_tokens(q2) == len(hist) - 1    # the whole processed history, in place: only the last token runs
    assert eng.prefix_cache_stats() == dict(active=1, hits=1, tokens=len(hist) - 1, copies=0)
    (qq, tok), = eng.infer()
    assert qq == q2 and tok == ids[n]
    eng.close()


def test_engines_without_the_feature_refuse(tmp_path):
    eng = InferenceEngine.from_ini(_ini(tmp_path, ret="true"))
    assert eng.model_info("lookup_decoding") == 0
    q = eng.add_query(PROMPT)
    with pytest.raises(EngineError, match="return_output_tensors"):
        eng.generate_lookup(q, 4)
    eng.close()
    eng = InferenceEngine.from_ini(_ini(tmp_path))
    q = eng.add_query(PROMPT, strategy="sample.top_p", seed=7)
    with pytest.raises(EngineError, match="greedily"):
        eng.generate_lookup(q, 4)
    with pytest.raises(EngineError, match="does not exist"):
        eng.generate_lookup(q + 50, 4)
    eng.close()
    for key, val in (("lookup_draft_len", 0), ("lookup_draft_len", 8), ("lookup_ngram_min", 0), ("lookup_ngram_max", 0)):
        with pytest.raises(EngineError, match=key.replace("_max", "").replace("_min", "")):
            InferenceEngine.from_ini(_ini(tmp_path, **{key: val}))
