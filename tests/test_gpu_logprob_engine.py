"""-m gpu: log-probabilities through the InferenceEngine -- the perplexity harness scoring its windows on the device
(return_output_tensors = false) against the reference tool's fixture and against the host path; queries with logprobs against
the float64 log-softmax of the worker's logits row of every step (the "logits" tap)."""
import ctypes as C
import os

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import engine_fixtures as fx
from tests.logprob_util import bound, lse_f64
from tests.test_perplexity_ref_fixture import FX, MAXLEN, SHAPE, STRIDE, TOKENS

pytestmark = pytest.mark.gpu


def _ppl_engine(tmp, ret):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="F16", kvd="F16", ctx=int(FX["ctx"]), s=SHAPE, seed=int(FX["seed"]),
                                std=float(FX["std"]), shared_classifier=False, ret=ret)
    return InferenceEngine.from_ini(ini)


def test_device_perplexity_matches_the_reference_tool(tmp_path):
    """return_output_tensors = false and device scoring asked for: the windows are scored on the device.  (Without the feature
    there is no such call: on this engine the harness fails with "the engine returned no output tensor".)"""
    eng = _ppl_engine(tmp_path, "false")
    ppl, err, count = eng.perplexity(TOKENS, max_length=MAXLEN, stride=STRIDE, device_scoring=True)
    with pytest.raises(EngineError, match="return_output_tensors"):      # not asked for: the host path, which needs the tensors
        eng.perplexity(TOKENS, max_length=MAXLEN, stride=STRIDE)
    eng.close()
    assert count == int(FX["count"])
    assert abs(np.log(ppl) - np.log(float(FX["ppl"]))) <= 2e-3 * np.log(float(FX["ppl"])), (ppl, float(FX["ppl"]))
    assert abs(err - float(FX["err"])) <= 0.03 * float(FX["err"]), (err, float(FX["err"]))


def test_device_perplexity_against_the_host_path(tmp_path):
    """mean nll of the device path vs the return_output_tensors = true engine's: per token the kernel's bound + 2^-23 (the host's
    own float expf); the score() call returns the same per-token values the device path sums"""
    dev = _ppl_engine(tmp_path / "dev", "false")
    ppl_d, err_d, count_d = dev.perplexity(TOKENS, max_length=MAXLEN, stride=STRIDE, device_scoring=True)
    lps = [dev.score(TOKENS[s:s + MAXLEN]) for s in range(0, len(TOKENS), STRIDE) if len(TOKENS[s:s + MAXLEN]) >= 2]
    dev.close()
    host = _ppl_engine(tmp_path / "host", "true")
    ppl_h, err_h, count_h = host.perplexity(TOKENS, max_length=MAXLEN, stride=STRIDE)
    with pytest.raises(EngineError, match="return_output_tensors = false"):
        host.perplexity(TOKENS, max_length=MAXLEN, stride=STRIDE, device_scoring=True)
    # the per-token tolerance needs each row's lse: the host engine's own output tensors of the same windows
    V, tols = SHAPE["vocab"], []
    for s0 in range(0, len(TOKENS), STRIDE):
        win = [int(t) for t in TOKENS[s0:s0 + MAXLEN]]
        if len(win) < 2:
            continue
        qid = host.add_query(win)
        assert qid > 0 and len(host.infer()) == 1
        rows = host.last_logits(qid)
        assert rows.shape == (len(win), V)
        tols += [bound(V, lse_f64(rows[i])) + 2.0 ** -23 for i in range(len(win) - 1)]
        assert host.remove_query(qid)
    host.close()
    assert count_d == count_h == int(FX["count"]) == len(tols)
    tol = float(np.mean(tols))                                      # (a mean of per-token errors is at most the mean of their bounds)
    print("mean nll device %.9f host %.9f diff %.3e tol %.3e" % (np.log(ppl_d), np.log(ppl_h), abs(np.log(ppl_d) - np.log(ppl_h)), tol))
    assert abs(np.log(ppl_d) - np.log(ppl_h)) <= tol
    flat = np.concatenate(lps).astype(np.float64)
    assert flat.size == count_d and abs(-flat.mean() - np.log(ppl_d)) <= 2.0 ** -20      # (score() rounds lse - logit to float once)


def _tap(eng, n_rows, V):
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    p, n = C.c_void_p(), C.c_size_t()
    ia.check(L.ifa_model_get_buffer(C.c_void_p(h), b"logits", 0, C.byref(p), C.byref(n)))
    out = np.empty(n_rows * V, np.float16)
    ia.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, None))
    ia.check(L.ifa_stream_sync(None))
    return out.reshape(n_rows, V)


def _engine(tmp, pool_key="true", ret="false", maxq=6):
    ini, _ = fx.write_model_dir(str(tmp), fmt="llama2.c", wd="Q4", kvd="F16", ret=ret, maxq=maxq)
    if pool_key is not None:
        text = open(ini).read().replace("return_output_tensors = %s" % ret, "return_output_tensors = %s\ndevice_sampling_pool = %s" % (ret, pool_key))
        open(ini, "w").write(text)
    return InferenceEngine.from_ini(ini)


PROMPT = [int(t) for t in np.random.default_rng(5).integers(3, 1000, 7)]
V = 1000


def _check_row(row, chosen_tok, chosen_lp, top, n_top, what):
    """chosen / top logprobs against float64 log_softmax of the step's row; top = the n best offered ids (id 0, unk, is never offered)"""
    lse = lse_f64(row)
    tol = bound(V, lse)
    assert abs(chosen_lp - (float(row[chosen_tok]) - lse)) <= tol, (what, chosen_lp, float(row[chosen_tok]) - lse)
    offered = row.astype(np.float32).copy(); offered[0] = -np.inf
    order = sorted(range(V), key=lambda i: (-offered[i], i))[:n_top]
    assert [i for i, _ in top] == order, (what, top, order)
    for i, lp in top:
        assert abs(lp - (float(row[i]) - lse)) <= tol, (what, i)
    assert all(a[1] >= b[1] for a, b in zip(top, top[1:]))


def _run(eng, strategy, seed, logprobs, steps, prompt=PROMPT):
    qid = eng.add_query(prompt, strategy=strategy, seed=seed, logprobs=logprobs)
    assert qid > 0, eng._err()
    toks = []
    for step in range(steps):
        (q, tok), = eng.infer()
        if logprobs >= 0:
            row = _tap(eng, len(prompt) if step == 0 else 1, V)[-1]
            chosen, top = eng.last_logprobs(qid)
            assert len(top) == logprobs
            _check_row(row, tok, chosen, top, logprobs, (strategy, step))
        else:
            with pytest.raises(EngineError):
                eng.last_logprobs(qid)
        toks.append(tok)
        assert eng.commit({qid: tok})
    assert eng.remove_query(qid)
    return toks


@pytest.mark.parametrize("pool_key", ["true", None])
def test_decode_logprobs_single_query(tmp_path, pool_key):
    eng = _engine(tmp_path, pool_key)
    for strategy, seed in ((None, 0), ("greedy", 0), ("sample.top_p", 17)):
        if strategy == "sample.top_p" and pool_key is None:
            continue      # (without device_sampling_pool the plain run's sampled steps take the op-by-op layer: another step's logits)
        plain = _run(eng, strategy, seed, -1, 10)
        assert _run(eng, strategy, seed, 5, 10) == plain, strategy
        assert _run(eng, strategy, seed, 0, 10) == plain, strategy
        assert _run(eng, strategy, seed, 20, 4) == plain[:4], strategy
    if pool_key is None:      # sampled + logprobs without the key still works and is self-consistent (checked against its own rows)
        a = _run(eng, "sample.top_p", 17, 5, 10)
        assert _run(eng, "sample.top_p", 17, 5, 10) == a
    # option parsing
    for bad in (-2, 21, 100):
        assert eng.add_query(PROMPT, logprobs=bad) < 0 and "logprobs" in eng._err()
    assert eng.query_count() == 0
    eng.close()


def test_decode_logprobs_two_queries_batched(tmp_path):
    eng = _engine(tmp_path, "true")

    def run(lp1, lp2):
        q1 = eng.add_query(PROMPT, strategy="sample.top_p", seed=31, logprobs=lp1)
        q2 = eng.add_query(PROMPT[:5], logprobs=lp2)
        assert q1 > 0 and q2 > 0
        order = sorted([q1, q2])
        res = dict(eng.infer())                                  # the two prompt steps, one by one
        assert eng.commit(res)
        out = []
        for step in range(6):
            res = dict(eng.infer())
            assert set(res) == {q1, q2}
            rows = _tap(eng, 2, V)
            for q, lp in ((q1, lp1), (q2, lp2)):
                if lp >= 0:
                    chosen, top = eng.last_logprobs(q)
                    _check_row(rows[order.index(q)], res[q], chosen, top, lp, ("batched", step, q))
            out.append((res[q1], res[q2]))
            assert eng.commit(res)
        assert eng.remove_query(q1) and eng.remove_query(q2)
        return out

    plain = run(-1, -1)
    assert run(5, 5) == plain
    assert run(5, -1) == plain
    assert run(-1, 0) == plain
    eng.close()


def test_logprobs_need_the_rows_on_the_device(tmp_path):
    eng = _engine(tmp_path, None, ret="true")
    assert eng.add_query(PROMPT, logprobs=3) < 0 and "return_output_tensors" in eng._err()
    assert eng.add_query(PROMPT) > 0
    eng.close()
