"""-m gpu: InferenceEngine::GenerateBatch (generate_batch) against the Infer / CommitInferenceResult loop of a second engine on the
same model directory, token for token: each query of the loop is committed until it has its max_new_tokens and then left alone.
`batch_generate_round_steps = 4`, so several rounds run and queries drop out at round boundaries; the last live query finishes
through Generate's single-row path.  Greedy, seeded sampled and processed queries (the seeds and strategies of
tests/test_gpu_sampled_generate.py), four more loop steps on both engines for the generator / count hand-off, a Q8 cache, a query
that crosses max_context_len with the context shift on, stop ids, the counters, the refusals."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import engine_fixtures as fx
from tests.test_gpu_logit_processors_engine import OPTS, PROMPT

pytestmark = pytest.mark.gpu

ROUND = 4
_rng = np.random.default_rng(11)
PROMPTS = [PROMPT] + [[int(t) for t in _rng.integers(3, 1000, n)] for n in (5, 9, 3, 12, 6)]
BUDGETS = [10, 7, 13, 5, 9, 11]


def _engine(tmp, sampler=True, kvd="F16", shift=False, ret="false", devices="0"):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd=kvd, ret=ret, ctx=64, maxq=8, devices=devices)
    keys = "device_sampling_pool = true\nbatch_generate_round_steps = %d\n" % ROUND + ("device_sampler = true\n" if sampler else "") \
        + ("context_shift = true\n" if shift else "")
    text = open(ini).read().replace("return_output_tensors = %s" % ret, "return_output_tensors = %s\n" % ret + keys)
    open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    gen = _engine(tmp_path_factory.mktemp("gen"))
    loop = _engine(tmp_path_factory.mktemp("loop"), sampler=False)
    assert gen.model_info("batch_generate") == 1 and gen.model_info("device_sampler") == 1 and loop.model_info("device_sampler") == 0
    yield gen, loop
    gen.close()
    loop.close()


_LIVE = {}      # engine -> the ids a test added (a failed test must not leave the next one a full engine)


def _add(gen, loop, specs):
    """specs: [(prompt, add_query options)]; the same queries on both engines -> (ids on gen, ids on loop)"""
    for eng in (gen, loop):
        for q in _LIVE.pop(id(eng), []):
            eng.remove_query(q)
    a = [gen.add_query(p, **o) for p, o in specs]
    b = [loop.add_query(p, **o) for p, o in specs]
    _LIVE[id(gen)], _LIVE[id(loop)] = list(a), list(b)
    assert all(q > 0 for q in a + b), (gen._err(), loop._err())
    return a, b


def _loop(eng, budgets, keep_until=None):
    """the Infer / Commit loop: every query is committed until it has its budget and then left alone -- Infer steps every query that
    has a committed token pending, so the commit of a query's LAST token waits until the loop is over: the query then takes part in
    no further step (and draws nothing more), which is where GenerateBatch leaves it.  keep_until {qid: n}: the query goes on being
    committed until it has n tokens (a stopped query stays in its round); only its first budget tokens are returned"""
    target = {q: max(n, (keep_until or {}).get(q, 0)) for q, n in budgets.items()}
    got, held = {q: [] for q in budgets}, {}
    while any(len(got[q]) < target[q] for q in budgets):
        items = dict(eng.infer())
        step = {q: tok for q, tok in items.items() if q in got and len(got[q]) < target[q]}
        assert step, items
        commit = {}
        for q, tok in step.items():
            got[q].append(tok)
            (held if len(got[q]) == target[q] else commit)[q] = tok
        assert not commit or eng.commit(commit)
    assert not held or eng.commit(held)
    return {q: got[q][:budgets[q]] for q in budgets}


def _more(eng, ids, steps=4):
    out = []
    for _ in range(steps):
        items = dict(eng.infer())
        out.append([items[q] for q in ids])
        assert eng.commit({q: items[q] for q in ids})
    return out


def _logit_state(eng):
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    p, n = C.c_void_p(), C.c_size_t()
    ia.check(L.ifa_model_get_buffer(C.c_void_p(h), b"logit_state", 0, C.byref(p), C.byref(n)))
    out = np.empty(n.value, np.uint8)
    ia.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, n.value, None))
    ia.check(L.ifa_stream_sync(None))
    return out


def _equal_run(gen, loop, specs, budgets, stats_out=None):
    a, b = _add(gen, loop, specs)
    got, stopped, stats = gen.generate_batch([(q, n) for q, n in zip(a, budgets)])
    want = _loop(loop, dict(zip(b, budgets)))
    for qa, qb in zip(a, b):
        assert got[qa] == want[qb], (qa, got[qa], want[qb])
        assert not stopped[qa] and gen.query_rng_state(qa) == loop.query_rng_state(qb)
    assert _more(gen, a) == _more(loop, b)                 # generator, counts and cache rows went on where the loop's stand
    if stats_out is not None:
        stats_out.update(stats)
    return a, b, got


def _remove(gen, loop, a, b):
    for q in a:
        assert gen.remove_query(q)
    for q in b:
        assert loop.remove_query(q)


@pytest.mark.parametrize("n", [2, 3, 6])
def test_greedy_queries_equal_the_loop(engines, n):
    gen, loop = engines
    rounds0, steps0 = gen.model_info("batch_generate_rounds"), gen.model_info("batch_generate_steps")
    stats = {}
    a, b, got = _equal_run(gen, loop, [(p, {}) for p in PROMPTS[:n]], BUDGETS[:n], stats)
    assert [len(got[q]) for q in a] == BUDGETS[:n]
    # the prefill yields token 1; rounds of at most 4 steps while two queries live; the last live query finishes alone
    assert stats["rounds"] >= 2 and stats["single_steps"] > 0 and stats["batched_steps"] <= ROUND * stats["rounds"]
    assert gen.model_info("batch_generate_rounds") - rounds0 == stats["rounds"] and gen.model_info("batch_generate_steps") - steps0 == stats["batched_steps"]
    more, _, _ = gen.generate_batch([(q, 3) for q in a])   # another call continues the queries
    want = _loop(loop, {q: 3 for q in b})
    assert [more[q] for q in a] == [want[q] for q in b]
    _remove(gen, loop, a, b)


def _mixed_specs():
    return [(PROMPTS[0], dict(strategy="sample.top_p", seed=4321)), (PROMPTS[1], dict(strategy="top_k", seed=17)),
            (PROMPTS[2], dict(strategy="sample.top_p", seed=17, **OPTS)), (PROMPTS[3], {}),
            (PROMPTS[4], dict(strategy="greedy", **OPTS)), (PROMPTS[5], dict(strategy="min_p", seed=99, temperature=1.3))]


def test_sampled_and_processed_queries_equal_the_loop(engines):
    gen, loop = engines
    drawn0, proc0 = gen.model_info("device_sampled_steps"), gen.model_info("processed_steps")
    a, b, got = _equal_run(gen, loop, _mixed_specs(), [12, 9, 12, 7, 10, 12])
    assert np.array_equal(_logit_state(gen), _logit_state(loop))
    assert len(set(got[a[0]] + got[a[1]] + got[a[5]])) > 3 and 400 not in got[a[2]] + got[a[4]]
    # one device-drawn step per emitted token behind each query's prompt step (the 4 loop steps of _more are the host's)
    assert gen.model_info("device_sampled_steps") - drawn0 == (12 - 1) + (9 - 1) + (12 - 1) + (10 - 1) + (12 - 1)
    assert gen.model_info("processed_steps") - proc0 >= (12 - 1) + (10 - 1)
    _remove(gen, loop, a, b)


def test_with_a_q8_cache(tmp_path):
    gen, loop = _engine(tmp_path / "a", kvd="Q8"), _engine(tmp_path / "b", sampler=False, kvd="Q8")
    _equal_run(gen, loop, _mixed_specs()[:3], [9, 12, 6])
    gen.close()
    loop.close()


def test_across_a_context_shift(tmp_path):
    gen, loop = _engine(tmp_path / "a", shift=True), _engine(tmp_path / "b", sampler=False, shift=True)
    n = 64 - len(PROMPTS[0]) + 9                           # query 0 runs past max_context_len = 64
    a, b, got = _equal_run(gen, loop, [(PROMPTS[0], dict(strategy="sample.top_p", seed=5)), (PROMPTS[1], {}), (PROMPTS[2], {})], [n, n - 3, 20])
    assert gen.model_info("context_shifts") == loop.model_info("context_shifts") >= 1
    assert [gen.query_shifted_tokens(q) for q in a] == [loop.query_shifted_tokens(q) for q in b] and gen.query_shifted_tokens(a[0]) > 0
    gen.close()
    loop.close()


def test_stop_ids(engines):
    gen, loop = engines
    specs, budgets = _mixed_specs()[:4], [12, 12, 12, 12]
    # the unstopped run tells which tokens to stop at (query 3 takes only its prompt step's token there, so the rounds have the
    # same three rows as below)
    a, b = _add(gen, loop, specs)
    free, _, _ = gen.generate_batch(list(zip(a, [12, 12, 12, 1])))
    for q in a:
        assert gen.remove_query(q)
    free = [free[q] for q in a]
    # query 1 stops inside the second round (token index 6 of 12: the prefill's token, round 1 = tokens 1..4, round 2 = tokens 5..8),
    # query 3 at the token of its prompt step
    at = next(i for i in (6, 5, 7) if free[1][i] not in free[1][:i])
    stops = {1: [2, free[1][at]], 3: [free[3][0]]}
    a = [gen.add_query(p, **o) for p, o in specs]
    got, stopped, _ = gen.generate_batch([(q, n, stops.get(i)) for i, (q, n) in enumerate(zip(a, budgets))])
    assert got[a[1]] == free[1][:at + 1] and stopped[a[1]] and got[a[3]] == free[3][:1] and stopped[a[3]]
    assert not stopped[a[0]] and not stopped[a[2]]
    # the loop: query 3 never joins a round; query 1 stays in its round (n does not change) and is lost at the round boundary
    want = _loop(loop, {b[0]: 12, b[1]: at + 1, b[2]: 12}, keep_until={b[1]: 9})
    assert got[a[0]] == want[b[0]] and got[a[2]] == want[b[2]] and got[a[1]] == want[b[1]]
    assert got[a[0]][:9] == free[0][:9] and got[a[2]][:9] == free[2][:9]      # the round of the stop is the unstopped run's
    assert gen.query_rng_state(a[0]) == loop.query_rng_state(b[0]) and gen.query_rng_state(a[2]) == loop.query_rng_state(b[2])
    _remove(gen, loop, a, b)


def test_refusals_touch_nothing(engines, tmp_path):
    gen, loop = engines
    a, b = _add(gen, loop, _mixed_specs()[:3])
    bad = gen.add_query(PROMPTS[3], strategy="mirostat", seed=3)
    assert bad > 0
    before = [gen.query_rng_state(q) for q in a]
    for items, word in (([(a[0], 4), (a[1], 4), (a[0], 2)], "given twice"), ([(a[0], 4), (9999, 4)], "does not exist"),
                        ([(a[0], 4), (a[1], 4, list(range(9)))], "stop ids"), ([(a[0], 4), (bad, 4)], "mirostat"),
                        ([(a[0], 4), (a[1], 200)], "exceed max_context_len"), ([(a[0], 4), (a[1], -1)], "max_new_tokens")):
        with pytest.raises(EngineError, match=word):
            gen.generate_batch(items)
    assert [gen.query_rng_state(q) for q in a] == before
    assert gen.remove_query(bad)
    got, _, _ = gen.generate_batch([(q, 6) for q in a])   # untouched: the queries still run like the loop's
    want = _loop(loop, {q: 6 for q in b})
    assert [got[q] for q in a] == [want[q] for q in b]
    _remove(gen, loop, a, b)
    off = _engine(tmp_path / "off", sampler=False)
    q1, q2 = off.add_query(PROMPTS[0], strategy="sample.top_p", seed=3), off.add_query(PROMPTS[1])
    with pytest.raises(EngineError, match="greedily"):
        off.generate_batch([(q1, 4), (q2, 4)])
    off.close()
    for name, kw, word, info in (("tp", dict(devices="0&0"), "single-device", 0), ("ret", dict(ret="true"), "return_output_tensors", 0)):
        eng = _engine(tmp_path / name, **kw)
        assert eng.model_info("batch_generate") == info
        q1, q2 = eng.add_query(PROMPTS[0]), eng.add_query(PROMPTS[1])
        with pytest.raises(EngineError, match=word):
            eng.generate_batch([(q1, 4), (q2, 4)])
        eng.close()
