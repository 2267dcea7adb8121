"""-m gpu: logit processors through the InferenceEngine (the small llama2.c Q4 model of tests/engine_fixtures.py, V = 1000): every
step's adjusted row (the worker's "logits_adj" tap) against the numpy restatement applied to the raw row (the "logits" tap) with
the host-tracked prompt / generated counts; tokens, logprobs, bans, the batched step, refusals, and an unprocessed query before
and after a processed one used its slot."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import engine_fixtures as fx
from tests.logit_adjust_util import PROMPT_BIT, restate
from tests.logprob_util import bound, lse_f64

pytestmark = pytest.mark.gpu

V = 1000
PROMPT = [int(t) for t in np.random.default_rng(5).integers(3, 1000, 7)]
PROMPT_B = [int(t) for t in np.random.default_rng(6).integers(3, 1000, 5)]
OPTS = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={PROMPT[0]: 5.0, 17: -100.0, 400: float("-inf")})
OPTS_B = dict(repetition_penalty=0.5, presence_penalty=-0.5, frequency_penalty=1.0)


def _engine(tmp, pool_key="true", ret="false", maxq=6):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd="F16", ret=ret, maxq=maxq)
    if pool_key is not None:
        text = open(ini).read().replace("return_output_tensors = %s" % ret, "return_output_tensors = %s\ndevice_sampling_pool = %s" % (ret, pool_key))
        open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


def _tap(eng, name, n_rows):
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    p, n = C.c_void_p(), C.c_size_t()
    ia.check(L.ifa_model_get_buffer(C.c_void_p(h), name.encode(), 0, C.byref(p), C.byref(n)))
    assert p.value and (name == "logits" or n.value >= n_rows * V * 2), (name, p.value, n.value)      # ("logits" reports one row's bytes)
    out = np.empty(n_rows * V, np.float16)
    ia.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, None))
    ia.check(L.ifa_stream_sync(None))
    return out.reshape(n_rows, V)


class Tracker:
    """the host's view of a processed query's device state"""

    def __init__(self, prompt, opts):
        self.state = np.zeros(V, np.uint32)
        self.state[np.array(prompt)] |= PROMPT_BIT
        self.bias = np.zeros(V, np.float32)
        for k, v in (opts.get("logit_bias") or {}).items():
            self.bias[k] = v
        self.p = np.array([opts.get("repetition_penalty", 1.0), opts.get("frequency_penalty", 0.0), opts.get("presence_penalty", 0.0)], np.float32)

    def adjusted(self, raw_row):
        return restate(raw_row, self.state, self.bias, self.p)

    def commit(self, tok):
        self.state[tok] += np.uint32(1)


def _greedy(adj_row):
    """the pool's best entry: id 0 (unk) is never offered, NaN never enters, the lower id wins among equals"""
    x = adj_row.astype(np.float32).copy()
    x[0] = -np.inf
    x[np.isnan(x)] = -np.inf
    return int(np.argmax(x))


@pytest.mark.parametrize("strategy,seed", [("greedy", 0), ("sample.top_p", 17)])
def test_stepwise_adjusted_rows_tokens_and_logprobs(tmp_path, strategy, seed):
    eng = _engine(tmp_path)
    assert eng.model_info("logit_processors") == 1 and eng.model_info("processed_steps") == 0
    qid = eng.add_query(PROMPT, strategy=strategy, seed=seed, logprobs=5, **OPTS)
    assert qid > 0, eng._err()
    tr = Tracker(PROMPT, OPTS)
    toks = []
    for step in range(12):
        (q, tok), = eng.infer()
        raw = _tap(eng, "logits", len(PROMPT) if step == 0 else 1)[-1]
        adj = _tap(eng, "logits_adj", 1)[0]
        want = tr.adjusted(raw)
        bad = np.nonzero(adj.view(np.uint16) != want)[0]
        assert bad.size == 0, (step, bad[:8], adj.view(np.uint16)[bad[:8]], want[bad[:8]])
        assert adj[400] == -np.inf and tok != 400
        if strategy == "greedy":
            assert tok == _greedy(adj), (step, tok, _greedy(adj))
        chosen, top = eng.last_logprobs(qid)
        lse = lse_f64(adj)
        assert abs(chosen - (float(adj[tok]) - lse)) <= bound(V, lse), (step, chosen, float(adj[tok]) - lse)
        assert len(top) == 5 and top[0][0] == _greedy(adj)           # the candidates are those of the processed row
        toks.append(tok)
        assert eng.commit({qid: tok})
        tr.commit(tok)
    assert eng.model_info("processed_steps") == 12
    assert eng.remove_query(qid)
    # without logprobs: the same tokens (the pool and the draws do not depend on the lse riding along)
    qid = eng.add_query(PROMPT, strategy=strategy, seed=seed, **OPTS)
    again = []
    for step in range(12):
        (q, tok), = eng.infer()
        again.append(tok)
        assert eng.commit({qid: tok})
    assert again == toks
    eng.close()


def _run(eng, prompt, steps, strategy=None, seed=0, rows=None, **opts):
    qid = eng.add_query(prompt, strategy=strategy, seed=seed, **opts)
    assert qid > 0, eng._err()
    toks = []
    for step in range(steps):
        (q, tok), = eng.infer()
        if rows is not None:
            rows.append(_tap(eng, "logits", len(prompt) if step == 0 else 1)[-1].copy())
        toks.append(tok)
        assert eng.commit({qid: tok})
    assert eng.remove_query(qid)
    return toks


def test_a_banned_token_never_appears(tmp_path):
    eng = _engine(tmp_path, None)
    t0 = _run(eng, PROMPT, 1)[0]
    toks = _run(eng, PROMPT, 16, logit_bias={t0: float("-inf")})
    assert toks[0] != t0 and t0 not in toks, (t0, toks)
    eng.close()


def test_a_huge_presence_penalty_never_repeats(tmp_path):
    eng = _engine(tmp_path, None)
    toks = _run(eng, PROMPT, 24, presence_penalty=1000.0)
    assert len(set(toks)) == 24, toks
    eng.close()


def test_batched_step_of_processed_and_plain_queries(tmp_path):
    """4 queries in one batched step: two processed (greedy, sampled), one plain sampled, one plain greedy.  Every processed row of
    every step is checked against the restatement of ITS slot's state.  Tokens: a single-query step (int8 activations) and a batched
    step (F16 activations on the matrix cores) are different arithmetic in this engine with or without processors, and a sampled draw
    over this model's nearly flat rows follows the last bit -- so "alone" is taken at the same step shape: the unprocessed queries
    against the same four queries with nobody processed (the routes of a build without the feature), each processed query against
    the step in which it is the only processed one; the greedy processed query also against its own single-query run."""
    eng = _engine(tmp_path)
    specs = [dict(prompt=PROMPT, strategy="greedy", seed=0, opts=OPTS),
             dict(prompt=PROMPT_B, strategy="sample.top_p", seed=31, opts={}),
             dict(prompt=PROMPT_B, strategy="sample.top_p", seed=23, opts=OPTS_B),
             dict(prompt=PROMPT[:5], strategy="greedy", seed=0, opts={})]
    steps = 6

    def run(processed):
        opts = [s["opts"] if i in processed else {} for i, s in enumerate(specs)]
        qids = [eng.add_query(s["prompt"], strategy=s["strategy"], seed=s["seed"], **o) for s, o in zip(specs, opts)]
        assert all(q > 0 for q in qids), eng._err()
        trackers = [Tracker(s["prompt"], o) if o else None for s, o in zip(specs, opts)]
        got = [[] for _ in specs]
        res = dict(eng.infer())                                     # the four prompt steps, one by one
        for step in range(steps + 1):
            assert set(res) == set(qids)
            if step > 0 and processed:                              # a batched step: raw rows in query order
                raw = _tap(eng, "logits", 4)
                adj = _tap(eng, "logits_adj", 4)
                # the step's pooled rows, ascending: the processed and the sampled queries; "logits_adj" row j belongs to pooled row j
                pooled = [i for i, s in enumerate(specs) if trackers[i] is not None or s["strategy"] != "greedy"]
                for i, tr in enumerate(trackers):
                    if tr is None:
                        continue
                    j = pooled.index(i)
                    assert np.array_equal(adj[j].view(np.uint16), tr.adjusted(raw[i])), (step, i, j)
                    if specs[i]["strategy"] == "greedy":
                        assert res[qids[i]] == _greedy(adj[j])
            for i, q in enumerate(qids):
                got[i].append(res[q])
                if trackers[i] is not None:
                    trackers[i].commit(res[q])
            assert eng.commit(res)
            if step < steps:
                res = dict(eng.infer())
        for q in qids:
            assert eng.remove_query(q)
        return got

    before = eng.model_info("processed_steps")
    plain = run(())
    assert eng.model_info("processed_steps") == before              # nobody processed: nothing armed
    mixed = run((0, 2))
    assert mixed[1] == plain[1] and mixed[3] == plain[3], (mixed, plain)
    assert mixed[0] == run((0,))[0] and mixed[2] == run((2,))[2]
    assert mixed[0] != plain[0] and mixed[2] != plain[2]            # (the processors do change these rows' tokens)
    alone0 = _run(eng, specs[0]["prompt"], steps + 1, strategy="greedy", **OPTS)
    eng.close()
    assert mixed[0] == alone0, (mixed[0], alone0)


def _set_worker_option(eng, name, value):
    L = ia.lib()
    ia.check(L.ifa_model_set_option(C.c_void_p(L.ifa_engine_worker(eng._h, 0)), name.encode(), int(value)))


@pytest.mark.parametrize("option", ["perf_stat", "exact_order"])
def test_processors_behind_the_fallback_steps(tmp_path, option):
    """the worker options that swap the step for the op-by-op / order-exact one: the pool -- and the processors in front of it -- sit
    behind those steps too (prompt row by row under exact_order, then single-token steps)"""
    eng = _engine(tmp_path, None)
    _set_worker_option(eng, option, 1)
    qid = eng.add_query(PROMPT, logprobs=3, **OPTS)
    assert qid > 0, eng._err()
    tr = Tracker(PROMPT, OPTS)
    for step in range(4):
        (q, tok), = eng.infer()
        n_rows = len(PROMPT) if step == 0 and option != "exact_order" else 1       # (exact_order feeds the prompt row by row)
        raw = _tap(eng, "logits", n_rows)[-1]
        adj = _tap(eng, "logits_adj", 1)[0]
        assert np.array_equal(adj.view(np.uint16), tr.adjusted(raw)), (option, step)
        assert tok == _greedy(adj)
        chosen, top = eng.last_logprobs(qid)
        lse = lse_f64(adj)
        assert abs(chosen - (float(adj[tok]) - lse)) <= bound(V, lse)
        assert eng.commit({qid: tok})
        tr.commit(tok)
    eng.close()


def test_a_batched_step_taken_as_two_chunks(tmp_path):
    """34 queries: more than one fused batched step holds, so the worker runs two steps of 17 rows (chunk0 = 0 and 17) behind one
    call; every second query is processed.  "logits" holds the LAST chunk's raw rows, "logits_adj" every pooled row of the call: the
    last chunk's processed rows bit for bit, every processed query's token = the best entry of its adjusted row."""
    n = 34
    eng = _engine(tmp_path, None, maxq=40)
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(3, 1000, 4)] for _ in range(n)]
    opts = [dict(frequency_penalty=0.5 + 0.01 * i, repetition_penalty=1.2, logit_bias={5 + i: -100.0}) if i % 2 else {} for i in range(n)]
    qids = [eng.add_query(p, **o) for p, o in zip(prompts, opts)]
    assert all(q > 0 for q in qids), eng._err()
    trackers = [Tracker(p, o) if o else None for p, o in zip(prompts, opts)]
    pooled = [i for i in range(n) if trackers[i] is not None]       # greedy queries, no device_sampling_pool: only the processed rows
    res = dict(eng.infer(capacity=64))
    for step in range(3):
        assert set(res) == set(qids)
        if step > 0:
            raw = _tap(eng, "logits", 17)                           # rows 17 .. 33 of the call
            adj = _tap(eng, "logits_adj", len(pooled))
            for j, i in enumerate(pooled):
                assert res[qids[i]] == _greedy(adj[j]), (step, i)
                if i >= 17:
                    assert np.array_equal(adj[j].view(np.uint16), trackers[i].adjusted(raw[i - 17])), (step, i)
        for i, q in enumerate(qids):
            if trackers[i] is not None:
                trackers[i].commit(res[q])
        assert eng.commit(res)
        res = dict(eng.infer(capacity=64))
    eng.close()


def test_refusals(tmp_path):
    eng = _engine(tmp_path / "a", None)
    qid = eng.add_query(PROMPT, **OPTS)
    assert qid > 0
    with pytest.raises(EngineError, match="logit processors.*Infer / CommitInferenceResult"):
        eng.generate(qid, 4)
    with pytest.raises(EngineError, match="logit processors.*Infer / CommitInferenceResult"):
        eng.generate_lookup(qid, 4)
    assert eng.remove_query(qid)
    # values the engine refuses, each with its message
    for bad, word in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                      (dict(presence_penalty=float("nan")), "presence_penalty"), (dict(frequency_penalty=float("-inf")), "frequency_penalty"),
                      (dict(logit_bias={V: 1.0}), "outside the vocabulary"), (dict(logit_bias={3: float("inf")}), "finite or -inf"),
                      (dict(logit_bias={i: 1.0 for i in range(1, 1026)}), "1024")):
        assert eng.add_query(PROMPT, **bad) < 0 and word in eng._err(), (bad, eng._err())
    assert eng.query_count() == 0
    eng.close()
    ret = _engine(tmp_path / "b", None, ret="true")
    assert ret.model_info("logit_processors") == 0
    assert ret.add_query(PROMPT, presence_penalty=0.5) < 0 and "return_output_tensors" in ret._err()
    assert ret.add_query(PROMPT) > 0
    ret.close()


def test_an_unprocessed_query_is_untouched_by_a_processed_one_in_its_slot(tmp_path):
    eng = _engine(tmp_path, None)
    rows_a, rows_b = [], []
    before = _run(eng, PROMPT, 8, rows=rows_a)
    _run(eng, PROMPT, 8, **OPTS)                                # the same slot: the first free one
    after = _run(eng, PROMPT, 8, rows=rows_b)
    assert before == after
    for a, b in zip(rows_a, rows_b):
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert eng.model_info("processed_steps") == 8
    eng.close()
