"""-m gpu: the context shift through the InferenceEngine's C ABI (`context_shift = true`) on the tiny model with
max_context_len = 64: a query runs past the limit and its books are those the plan function predicts; its ids are those of a
worker-level replay that shifts by hand at the same moments -- one query, and three inside batched steps; Generate across the
limit returns the Infer / Commit loop's ids; the per-query options; what a shifted query leaves to the prefix cache; a processed
query across a shift; the service no longer cuts max_output_len down."""
import ctypes as C
import http.client
import json
import os
import subprocess

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import build
from inferflow_amd.engine import EngineError, InferenceEngine, context_shift_plan
from tests import engine_fixtures as fx
from tests.test_gpu_logit_processors_engine import Tracker, _greedy, _tap

pytestmark = pytest.mark.gpu

V, CTX, KEEP = fx.SHAPE["vocab"], 64, 4
RNG = np.random.default_rng(41)
PROMPT = [int(t) for t in RNG.integers(3, V, 10)]


def _inis(tmp, kvd="F16", extra="", ret="false", maxq=4):
    """(ini with context_shift = true [+ extra keys], ini without the key) over ONE model directory"""
    off, _ = fx.write_model_dir(str(tmp), wd="Q4", kvd=kvd, ret=ret, maxq=maxq, ctx=CTX)
    text = open(off).read()
    assert "dynamic_batching_min_queries = 2\n" in text
    on = os.path.join(str(tmp), "engine_on.ini")
    open(on, "w").write(text.replace("dynamic_batching_min_queries = 2\n", "dynamic_batching_min_queries = 2\ncontext_shift = true\n" + extra))
    return on, off


def _loop(eng, qids, n_steps):
    """n_steps x {Infer, Commit(greedy)}: {qid: ids}; a query that gets no item has ended"""
    out = {q: [] for q in qids}
    for _ in range(n_steps):
        res = dict(eng.infer())
        if not res:
            break
        assert eng.commit(res)
        for q, t in res.items():
            out[q].append(t)
    return out


def _predict(n_prompt, n_new, keep=KEEP, ctx=CTX):
    """(shifts, tokens dropped) of a query of n_prompt tokens over n_new steps, from the plan function"""
    T, shifts, dropped = n_prompt, 0, 0
    for _ in range(n_new):
        p = context_shift_plan(T, T - 1, ctx, keep)
        assert p is not None
        if p:
            assert p[0] == keep
            T -= p[1]; shifts += 1; dropped += p[1]
        T += 1
    return shifts, dropped


def test_a_query_runs_past_the_limit_only_with_the_key(tmp_path):
    on, off = _inis(tmp_path)
    eng = InferenceEngine.from_ini(off)
    assert eng.model_info("context_shift") == 0 and eng.model_info("context_shift_available") == 1
    q = eng.add_query(PROMPT)
    ids = _loop(eng, [q], 200)[q]
    assert len(ids) == CTX - len(PROMPT)                           # as before: ended at 64 tokens, no item afterwards
    assert eng.infer() == [] and eng.query_shifted_tokens(q) == 0 and eng.model_info("context_shifts") == 0
    eng.close()
    eng = InferenceEngine.from_ini(on)
    assert eng.model_info("context_shift") == 1
    q = eng.add_query(PROMPT)
    ids2 = _loop(eng, [q], 200)[q]
    assert len(ids2) == 200 and ids2[:len(ids)] == ids             # (the tokens in front of the first shift are the unshifted query's)
    shifts, dropped = _predict(len(PROMPT), 200)
    assert shifts >= 4 and dropped == 30 * shifts
    assert eng.query_shifted_tokens(q) == dropped and eng.query_shifted_tokens(q + 7) == -1
    assert eng.model_info("context_shifts") == shifts and eng.model_info("context_shift_tokens") == dropped
    eng.close()


class Hand:
    """the engine's worker, driven by hand"""

    def __init__(self, eng):
        self.L = ia.lib()
        self.h = C.c_void_p(self.L.ifa_engine_worker(eng._h, 0))

    def prompt(self, slot, toks):
        a = np.asarray(toks, np.int32)
        nxt = C.c_int(-1)
        ia.check(self.L.ifa_model_select_kv(self.h, slot))
        ia.check(self.L.ifa_model_forward(self.h, a.ctypes.data_as(C.c_void_p), a.size, 0, None, C.byref(nxt)))
        return nxt.value

    def step(self, slot, tok, pos):
        out = np.zeros(1, np.int32)
        ia.check(self.L.ifa_model_select_kv(self.h, slot))
        ia.check(self.L.ifa_model_decode(self.h, int(tok), int(pos), 1, out.ctypes.data_as(C.c_void_p), None))
        return int(out[0])

    def batch(self, toks, pos, slots):
        t, p, s = (np.asarray(x, np.int32) for x in (toks, pos, slots))
        out = np.zeros(t.size, np.int32)
        ia.check(self.L.ifa_model_decode_batch(self.h, t.size, t.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                               out.ctypes.data_as(C.c_void_p), None))
        return [int(x) for x in out]

    def shift(self, slot, keep, discard, n_rows):
        ia.check(self.L.ifa_model_kv_shift(self.h, slot, keep, discard, n_rows))


def _replay(hand, prompts, n_steps, keep=KEEP):
    """the engine's loop by hand: prompt steps, then single or batched greedy steps, kv_shift where the plan says so"""
    toks = [list(p) for p in prompts]
    out = [[] for _ in prompts]
    for slot, p in enumerate(prompts):
        t = hand.prompt(slot, p)
        toks[slot].append(t); out[slot].append(t)
    for _ in range(n_steps - 1):
        for slot, tk in enumerate(toks):
            plan = context_shift_plan(len(tk), len(tk) - 1, CTX, keep)
            if plan:
                hand.shift(slot, plan[0], plan[1], len(tk) - 1)
                del tk[plan[0]:plan[0] + plan[1]]
        if len(toks) == 1:
            nxt = [hand.step(0, toks[0][-1], len(toks[0]) - 1)]
        else:
            nxt = hand.batch([tk[-1] for tk in toks], [len(tk) - 1 for tk in toks], list(range(len(toks))))
        for slot, t in enumerate(nxt):
            toks[slot].append(t); out[slot].append(t)
    return out


@pytest.mark.parametrize("kvd", ["F16", "Q8"])
def test_ids_match_a_worker_level_replay(tmp_path, kvd):
    on, _ = _inis(tmp_path, kvd=kvd)
    eng = InferenceEngine.from_ini(on)
    # one query alone
    q = eng.add_query(PROMPT)
    ids = _loop(eng, [q], 130)[q]
    assert len(ids) == 130 and eng.query_shifted_tokens(q) == _predict(len(PROMPT), 130)[1] > 30
    assert eng.remove_query(q)
    assert _replay(Hand(eng), [PROMPT], 130)[0] == ids
    # three queries that reach the limit at different steps, inside batched steps
    prompts = [PROMPT, [int(t) for t in RNG.integers(3, V, 23)], [int(t) for t in RNG.integers(3, V, 37)]]
    qs = [eng.add_query(p) for p in prompts]
    assert all(x > 0 for x in qs), eng._err()
    got = _loop(eng, qs, 100)
    for q, p in zip(qs, prompts):
        assert len(got[q]) == 100 and eng.query_shifted_tokens(q) == _predict(len(p), 100)[1] > 0
    for q in qs:
        assert eng.remove_query(q)
    want = _replay(Hand(eng), prompts, 100)
    for i, q in enumerate(qs):
        assert got[q] == want[i], (kvd, i)
    eng.close()


def test_generate_across_the_limit_returns_the_infer_loops_ids(tmp_path):
    on, off = _inis(tmp_path)
    eng = InferenceEngine.from_ini(on)
    q = eng.add_query(PROMPT)
    want = _loop(eng, [q], 100)[q]
    assert _predict(len(PROMPT), 100)[0] == 2 and eng.query_shifted_tokens(q) == 60
    assert eng.remove_query(q)
    q = eng.add_query(PROMPT)
    got, _ = eng.generate(q, 100)
    assert [int(t) for t in got] == want and eng.query_shifted_tokens(q) == 60
    more, _ = eng.generate(q, 7)                                    # and it goes on from where it stands
    assert len(more) == 7
    assert eng.remove_query(q)
    # Infer steps, then Generate from inside the run, across the next limit
    q = eng.add_query(PROMPT)
    head = _loop(eng, [q], 20)[q]
    tail, _ = eng.generate(q, 80)
    assert head + [int(t) for t in tail] == want
    # lookup decoding crosses the limit too (its tokens are the rows route's: the count and the books are checked)
    ql = eng.add_query(PROMPT)
    toks, stats = eng.generate_lookup(ql, 100)
    assert len(toks) == 100 and eng.query_shifted_tokens(ql) >= 30 and stats["steps"] >= 1
    eng.close()
    eng = InferenceEngine.from_ini(off)                             # without the feature both still refuse
    q = eng.add_query(PROMPT)
    with pytest.raises(EngineError, match="exceed max_context_len"):
        eng.generate(q, 100)
    with pytest.raises(EngineError, match="exceed max_context_len"):
        eng.generate_lookup(q, 100)
    assert len(eng.generate(q, CTX - len(PROMPT))[0]) == CTX - len(PROMPT)
    eng.close()


def test_per_query_options(tmp_path):
    on, off = _inis(tmp_path)
    eng = InferenceEngine.from_ini(on)
    q0 = eng.add_query(PROMPT, context_shift=False)                 # off for this query on an engine with the key on
    assert q0 > 0, eng._err()
    assert len(_loop(eng, [q0], 200)[q0]) == CTX - len(PROMPT) and eng.query_shifted_tokens(q0) == 0
    assert eng.remove_query(q0)
    q1 = eng.add_query(PROMPT, context_keep=0)
    assert len(_loop(eng, [q1], 60)[q1]) == 60
    assert eng.query_shifted_tokens(q1) == _predict(len(PROMPT), 60, keep=0)[1] == 32
    assert eng.remove_query(q1)
    q2 = eng.add_query(PROMPT, context_keep=CTX // 2)
    assert q2 > 0 and len(_loop(eng, [q2], 60)[q2]) == 60 and eng.query_shifted_tokens(q2) == 16
    assert eng.remove_query(q2)
    assert eng.add_query(PROMPT, context_keep=CTX // 2 + 1) == -1 and "context_keep" in eng._err()
    assert eng.add_query(PROMPT, context_keep=-2) == -1
    assert eng.query_count() == 0
    eng.close()
    eng = InferenceEngine.from_ini(off)                             # on for this query on an engine with the key off
    q3 = eng.add_query(PROMPT, context_shift=True)
    assert q3 > 0, eng._err()
    assert len(_loop(eng, [q3], 70)[q3]) == 70 and eng.query_shifted_tokens(q3) == 30
    assert eng.remove_query(q3)
    # the explicit call, with the caller's own numbers
    q4 = eng.add_query(PROMPT)
    _loop(eng, [q4], 20)
    eng.shift_query(q4, 2, 5)
    assert eng.query_shifted_tokens(q4) == 5
    assert len(_loop(eng, [q4], 5)[q4]) == 5
    with pytest.raises(EngineError, match="ShiftQuery"):
        eng.shift_query(q4, 20, 20)                                 # more than it has processed
    with pytest.raises(EngineError):
        eng.shift_query(q4 + 50, 1, 1)
    eng.close()


def test_an_engine_that_cannot_shift_accepts_the_keys_and_stays_off(tmp_path):
    on, _ = _inis(tmp_path, ret="true")
    eng = InferenceEngine.from_ini(on)
    assert eng.model_info("context_shift") == 0 and eng.model_info("context_shift_available") == 0
    assert eng.add_query(PROMPT, context_shift=True) == -1 and "context shift" in eng._err()
    q = eng.add_query(PROMPT)
    assert len(_loop(eng, [q], 200)[q]) == CTX - len(PROMPT)
    with pytest.raises(EngineError):
        eng.shift_query(q, 1, 1)
    eng.close()


def test_a_shifted_query_leaves_only_its_kept_rows_to_the_prefix_cache(tmp_path):
    on, _ = _inis(tmp_path, extra="prefix_cache = true\ncontext_shift_keep = 20\n")
    eng = InferenceEngine.from_ini(on)
    assert eng.model_info("prefix_cache") == 1
    head = [int(t) for t in RNG.integers(3, V, 40)]
    q = eng.add_query(head + [7, 8, 9, 10, 11])
    _loop(eng, [q], 30)                                             # 45 + 30 tokens: one shift
    assert eng.query_shifted_tokens(q) == _predict(45, 30, keep=20)[1] > 0
    assert eng.remove_query(q)
    q2 = eng.add_query(head + [21, 22, 23])
    assert 0 <= eng.query_cached_tokens(q2) <= 20                   # at most the kept rows; the moved rows are no prompt's rows
    assert eng.query_cached_tokens(q2) == 20
    assert q2 in dict(eng.infer())
    assert eng.remove_query(q2)
    # a query that never shifted leaves its whole record, as before
    q3 = eng.add_query(head + [31, 32, 33, 34])
    assert eng.query_cached_tokens(q3) == 40                        # (q2's record: the 40 common tokens)
    _loop(eng, [q3], 3)
    assert eng.remove_query(q3)
    q4 = eng.add_query(head + [31, 32, 33, 34, 50])
    assert eng.query_cached_tokens(q4) == 44
    assert eng.remove_query(q4)
    eng.close()


def test_a_processed_query_keeps_counting_across_a_shift(tmp_path):
    """frequency_penalty over ALL generated tokens, the dropped ones included: every step's token is the greedy choice of the numpy
    restatement of the processors on the step's raw logits row"""
    on, _ = _inis(tmp_path)
    eng = InferenceEngine.from_ini(on)
    opts = dict(frequency_penalty=0.5)
    prompt = [int(t) for t in RNG.integers(3, V, 30)]
    q = eng.add_query(prompt, **opts)
    assert q > 0, eng._err()
    tr = Tracker(prompt, opts)
    for step in range(50):                                          # the limit is reached after 34 tokens
        (qq, tok), = eng.infer()
        raw = _tap(eng, "logits", len(prompt) if step == 0 else 1)[-1]
        assert tok == _greedy(tr.adjusted(raw).view(np.float16)), step
        assert eng.commit({q: tok})
        tr.commit(tok)
    assert eng.query_shifted_tokens(q) == _predict(len(prompt), 50)[1] == 30
    assert eng.model_info("processed_steps") == 50
    eng.close()


def test_the_service_does_not_cut_the_output_down(tmp_path):
    build.build_library()
    on, _ = _inis(tmp_path)
    eng = InferenceEngine.from_ini(on)
    q = eng.add_query(PROMPT)
    want = _loop(eng, [q], 150)[q]
    eng.close()
    exe = os.path.join(build.BIN_DIR, "ifa_service")
    p = subprocess.Popen([exe, on, "--port", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    try:
        line = p.stdout.readline()
        assert line.startswith("listening on 127.0.0.1:"), line
        port = int(line.strip().rsplit(":", 1)[1])

        def post(body):
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
            c.request("POST", "/", body=json.dumps(body), headers={"Content-Type": "application/json"})
            r = c.getresponse()
            data = json.loads(r.read().decode())
            c.close()
            return r.status, data
        st, r = post({"prompt_token_ids": PROMPT, "max_output_len": 150})
        assert st == 200 and r["ret_code"] == "succ" and r["token_ids"] == want, r
        st, r = post({"prompt_token_ids": PROMPT, "max_output_len": 150, "context_shift": False})
        assert r["ret_code"] == "succ" and r["token_ids"] == want[:CTX - len(PROMPT)]
        st, r = post({"prompt_token_ids": PROMPT, "max_output_len": 0})          # no positive bound: today's bound, it must still end
        assert r["ret_code"] == "succ" and len(r["token_ids"]) == CTX - len(PROMPT)
        st, r = post({"prompt_token_ids": list(range(3, 3 + CTX)), "max_output_len": 5})
        assert r["ret_code"] == "error.too_long_request"
    finally:
        p.terminate()
        p.wait(timeout=20)
