"""The verify chain of lookup decoding for sampled queries on the CPU: ifa_sample_verify_host (csrc/ifa_sample_verify.hip) against the
specification written in Python over W.sample_pool_host (tests/verify_cases.py:chain) -- every acceptance outcome at 1, 2, 5 and 8
rows, the generator hand-off (two steps per emitted token, none for greedy) and the error word.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from inferflow_amd import _capi, worker as W
from tests import sample_pools as P
from tests import verify_cases as V

ROWS = [1, 2, 5, 8]


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(_capi.library_path())
    for name in ("ifa_sample_verify_rows", "ifa_sample_verify_host", "ifa_logit_adjust_draft_rows", "ifa_model_decode_draft_sampled"):
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    for name in ("sample_verify_rows", "sample_verify_host", "logit_adjust_draft_rows"):
        assert callable(getattr(W, name)), name
    assert callable(W.DecodeWorker.decode_draft_sampled)


def _pools(rows, kind, salt):
    if kind == "natural":
        nat = [(i, b) for _, i, b in P.natural_pools()]
        return [nat[(salt + 17 * r) % len(nat)] for r in range(rows)]
    if kind == "ties":
        return V.tie_pools(rows, salt)
    return V.pools_of_length({"one": 1, "big": 256}[kind], rows, salt)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", ["natural", "ties", "one", "big"])
def test_host_chain_equals_the_python_chain(rows, kind):
    n_cases = 0
    for si, combo in enumerate(V.STRATEGIES):
        params = W.sample_params_array([combo])
        for mismatch in V.mismatch_rows(rows):
            pools = _pools(rows, kind, 3 * si + (mismatch or 0))
            state0 = P.java_random_state(400 + 31 * si + rows)
            draft = V.drafts_for(pools, params[0], state0, mismatch)
            counts, ids, vals = V.arrays(pools, 256 if si % 2 else None)
            want = V.chain(pools, params[0], state0, draft)
            got = W.sample_verify_host(counts, ids, vals, params[0], draft, state0)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], (combo, mismatch, got, want)
            # the outcome the case was built for, and the generator: two steps per emitted token, none for greedy
            e = rows if mismatch is None else mismatch + 1
            assert got[2] == e and got[4] == 0 and np.all(got[0][:e] >= 0) and np.all(got[0][e:] == -1)
            assert got[3] == (state0 if combo[0] == P.GREEDY else V.advance(state0, 2 * e))
            n_cases += 1
    assert n_cases == len(V.STRATEGIES) * len(V.mismatch_rows(rows))


@pytest.mark.parametrize("combo", [V.STRATEGIES[2], V.STRATEGIES[4]])
def test_an_empty_pool_fails_only_where_the_chain_reaches_it(combo):
    rows, empty = 5, 3
    params = W.sample_params_array([combo])
    pools = _pools(rows, "natural", 9)
    pools[empty] = (np.zeros(0, np.int32), np.zeros(0, np.uint16))
    state0 = P.java_random_state(77)
    counts, ids, vals = V.arrays(pools, 64)
    # reached: rows 0 .. empty - 1 accepted
    full = [(i, b) if len(i) else pools[0] for i, b in pools]
    draft = V.drafts_for(full, params[0], state0, None)
    toks, idx, n_out, st, err = W.sample_verify_host(counts, ids, vals, params[0], draft, state0)
    assert (n_out, err) == (empty, empty + 1) and np.all(toks[empty:] == -1) and np.array_equal(toks[:empty], draft[:empty])
    assert st == (state0 if combo[0] == P.GREEDY else V.advance(state0, 2 * empty))
    want = V.chain(pools, params[0], state0, draft)
    assert np.array_equal(toks, want[0]) and (n_out, st, err) == want[2:]
    # an error word that is set already is left alone
    assert W.sample_verify_host(counts, ids, vals, params[0], draft, state0, err=42)[4] == 42
    # behind the first mismatch: never looked at
    draft2 = draft.copy()
    draft2[1] += 1
    toks, idx, n_out, st, err = W.sample_verify_host(counts, ids, vals, params[0], draft2, state0)
    assert (n_out, err) == (2, 0) and st == (state0 if combo[0] == P.GREEDY else V.advance(state0, 4))


def test_an_unknown_strategy_fails_row_0():
    pools = _pools(2, "natural", 1)
    counts, ids, vals = V.arrays(pools)
    params = W.sample_params_array([(5, 1.0, 0.9, 8, 0.05)])
    toks, idx, n_out, st, err = W.sample_verify_host(counts, ids, vals, params[0], [1], 12345)
    assert (n_out, st, err) == (0, 12345, 1) and np.all(toks == -1)


def test_arguments_are_checked():
    pools = _pools(2, "natural", 1)
    counts, ids, vals = V.arrays(pools)
    params = W.sample_params_array([V.STRATEGIES[0]])
    with pytest.raises(_capi.IfaError, match="rows 9 outside 1..8"):
        W.sample_verify_host(np.zeros(9, np.int32), np.zeros((9, 4), np.int32), np.zeros((9, 4), np.uint16), params[0], np.zeros(8, np.int32), 1)


def test_the_ini_key_parses_and_is_inert_without_the_device_sampler(tmp_path):
    """`lookup_sampled = true` gets through LoadConfig: without a device Init stops at the device check (never at the key); with one
    the engine comes up and -- device_sampler being off -- reports the feature inactive"""
    from inferflow_amd.engine import EngineError, InferenceEngine
    from tests import engine_fixtures as fx
    ini, _ = fx.write_model_dir(str(tmp_path), fmt="llama2.c", wd="Q4", kvd="F16", ret="false")
    text = open(ini).read()
    assert "return_output_tensors = false" in text
    open(ini, "w").write(text.replace("return_output_tensors = false", "return_output_tensors = false\nlookup_sampled = true"))
    try:
        eng = InferenceEngine.from_ini(ini)
    except EngineError as e:
        assert "not available" in str(e), e
        return
    assert eng.model_info("device_sampler") == 0 and eng.model_info("lookup_decoding") == 1
    assert eng.model_info("lookup_sampled") == 0 and eng.model_info("lookup_sampled_steps") == 0
    eng.close()


def test_engine_symbols_are_exported_and_bound():
    from inferflow_amd.engine import InferenceEngine
    lib = C.CDLL(_capi.library_path())
    assert hasattr(lib, "ifa_engine_query_rng_state") and "ifa_engine_query_rng_state" in _capi.ENGINE_SIGNATURES
    assert callable(InferenceEngine.query_rng_state)
