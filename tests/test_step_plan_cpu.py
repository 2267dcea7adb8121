"""CPU-only checks of the engine's step routes (host/step_plan.h) through the host-only entry points ifa_step_plan_query and
ifa_step_plan_batch: which worker call a step of InferenceEngine::Infer takes, what it brings to the host, when it is refused.
Tables only; the expected values are written out from the rule tables of DESIGN.md, not computed."""
import ctypes as C

import pytest

import inferflow_amd as ia
from inferflow_amd import _capi

MULTI, DECODE_POOL, FORWARD_POOL, DECODE, FORWARD = range(5)      # StepRoute
NONE, ALL_ROWS, LAST_ROW = range(3)                               # LogitsCopy
POOL_MAX = 256                                                    # IFA_POOL_MAX

# (multi, return_output_tensors, pool_route, sampled, n_new) -> (route, logits_rows, copy)
QUERY_TABLE = [
    # a single device, off the pool route
    ((0, 0, 0, 0, 1), (DECODE, 0, NONE)),
    ((0, 0, 0, 0, 2), (FORWARD, 0, NONE)),
    ((0, 0, 0, 1, 1), (FORWARD, 1, LAST_ROW)),
    ((0, 0, 0, 1, 2), (FORWARD, 2, LAST_ROW)),
    ((0, 1, 0, 0, 1), (FORWARD, 1, ALL_ROWS)),
    ((0, 1, 0, 0, 2), (FORWARD, 2, ALL_ROWS)),
    ((0, 1, 0, 1, 1), (FORWARD, 1, ALL_ROWS)),
    ((0, 1, 0, 1, 2), (FORWARD, 2, ALL_ROWS)),
    # a single device, on the pool route: nothing comes to the host; a prompt keeps its rows on the device
    ((0, 0, 1, 0, 1), (DECODE_POOL, 0, NONE)),
    ((0, 0, 1, 0, 2), (FORWARD_POOL, 2, NONE)),
    ((0, 0, 1, 1, 1), (DECODE_POOL, 0, NONE)),
    ((0, 0, 1, 1, 2), (FORWARD_POOL, 2, NONE)),
    ((0, 1, 1, 0, 1), (DECODE_POOL, 0, NONE)),
    ((0, 1, 1, 0, 2), (FORWARD_POOL, 2, NONE)),
    ((0, 1, 1, 1, 1), (DECODE_POOL, 0, NONE)),
    ((0, 1, 1, 1, 2), (FORWARD_POOL, 2, NONE)),
    # several devices: always the ranks' step, whatever pool_route says; the shards come over for tensors or host sampling
    ((1, 0, 0, 0, 1), (MULTI, 0, NONE)),
    ((1, 0, 0, 0, 2), (MULTI, 0, NONE)),
    ((1, 0, 0, 1, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 0, 0, 1, 2), (MULTI, 2, ALL_ROWS)),
    ((1, 1, 0, 0, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 1, 0, 0, 2), (MULTI, 2, ALL_ROWS)),
    ((1, 1, 0, 1, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 1, 0, 1, 2), (MULTI, 2, ALL_ROWS)),
    ((1, 0, 1, 0, 1), (MULTI, 0, NONE)),
    ((1, 0, 1, 0, 2), (MULTI, 0, NONE)),
    ((1, 0, 1, 1, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 0, 1, 1, 2), (MULTI, 2, ALL_ROWS)),
    ((1, 1, 1, 0, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 1, 1, 0, 2), (MULTI, 2, ALL_ROWS)),
    ((1, 1, 1, 1, 1), (MULTI, 1, ALL_ROWS)),
    ((1, 1, 1, 1, 2), (MULTI, 2, ALL_ROWS)),
]


def plan_query(multi, rot, pool_route, sampled, n_new):
    out = (C.c_int * 3)(-7, -7, -7)
    assert ia.lib().ifa_step_plan_query(multi, rot, pool_route, sampled, n_new, out) == 0
    return tuple(out)


def plan_batch(rot, rows):
    n = len(rows)
    flat = (C.c_int * (5 * n))(*[v for row in rows for v in row])
    pool_rows = (C.c_int * n)(*([-7] * n))
    out = (C.c_int * 5)(*([-7] * 5))
    assert ia.lib().ifa_step_plan_batch(rot, flat, n, pool_rows, out) == 0
    n_pool, pool_k, with_lse, want_logits, error_row = out
    assert 0 <= n_pool <= n
    assert all(pool_rows[i] == -7 for i in range(n_pool, n)), "nothing is written past the pool rows"
    return {"pool_rows": [pool_rows[i] for i in range(n_pool)], "pool_k": pool_k, "with_lse": with_lse, "want_logits": want_logits,
            "error_row": error_row}


def test_symbols_exported_and_bound():
    L = ia.lib()
    for name in ("ifa_step_plan_query", "ifa_step_plan_batch"):
        assert hasattr(L, name), "missing symbol " + name
        assert name in _capi.ENGINE_SIGNATURES


def test_query_table_is_complete():
    assert len(QUERY_TABLE) == 32
    assert sorted(k for k, _ in QUERY_TABLE) == [(m, t, p, s, n) for m in (0, 1) for t in (0, 1) for p in (0, 1) for s in (0, 1) for n in (1, 2)]


@pytest.mark.parametrize("inputs,expect", QUERY_TABLE)
def test_query_step(inputs, expect):
    assert plan_query(*inputs) == expect


GREEDY = (0, 0, 0, 0, 0)        # (pool_route, sampled, pool_len, pool_k, wants_logprobs)
BATCH_TABLE = [
    ("two greedy rows", 0, [GREEDY, GREEDY],
     {"pool_rows": [], "pool_k": 0, "with_lse": 0, "want_logits": 0, "error_row": -1}),
    ("pool row and greedy row", 0, [(1, 1, 40, 40, 0), GREEDY],
     {"pool_rows": [0], "pool_k": 40, "with_lse": 0, "want_logits": 0, "error_row": -1}),
    ("pool row and host-sampled row, no logprobs: the block comes over, nobody gets a pool", 0, [(1, 1, 40, 40, 0), (0, 1, 300, 300, 0)],
     {"pool_rows": [], "pool_k": 0, "with_lse": 0, "want_logits": 1, "error_row": -1}),
    ("greedy logprobs row and host-sampled row: the sampled row takes a pool too", 0, [(1, 0, 1, 5, 1), (0, 1, 40, 40, 0)],
     {"pool_rows": [0, 1], "pool_k": 40, "with_lse": 1, "want_logits": 0, "error_row": -1}),
    ("pool 10, pool + logprobs 50, greedy", 0, [(1, 1, 10, 10, 0), (1, 1, 50, 50, 1), GREEDY],
     {"pool_rows": [0, 1], "pool_k": 50, "with_lse": 1, "want_logits": 0, "error_row": -1}),
    ("return_output_tensors, one sampled and one greedy row, none on the pool route", 1, [(0, 1, 40, 40, 0), GREEDY],
     {"pool_rows": [], "pool_k": 0, "with_lse": 0, "want_logits": 1, "error_row": -1}),
]


@pytest.mark.parametrize("name,rot,rows,expect", BATCH_TABLE, ids=[c[0].split(":")[0] for c in BATCH_TABLE])
def test_batch_step(name, rot, rows, expect):
    assert plan_batch(rot, rows) == expect


@pytest.mark.parametrize("pool_len", [POOL_MAX + 1, 0])
def test_batch_refuses_a_host_sampled_row_without_a_device_pool_next_to_logprobs(pool_len):
    # the logprobs row needs its pool and lse, so the sampled row cannot bring the block over: it needs a pool of 1 .. IFA_POOL_MAX
    plan = plan_batch(0, [(1, 0, 1, 5, 1), (0, 1, pool_len, pool_len, 0)])
    assert plan["error_row"] == 1


def test_batch_pool_limit_is_inclusive_and_rows_stay_in_order():
    plan = plan_batch(0, [(0, 1, POOL_MAX, POOL_MAX, 0), GREEDY, (1, 0, 1, 5, 1), (0, 1, 1, 1, 0)])
    assert plan == {"pool_rows": [0, 2, 3], "pool_k": POOL_MAX, "with_lse": 1, "want_logits": 0, "error_row": -1}


def test_bad_arguments():
    L = ia.lib()
    out3 = (C.c_int * 3)()
    assert L.ifa_step_plan_query(0, 0, 0, 0, 0, out3) == -1            # a step of no tokens
    assert b"ifa_step_plan_query" in L.ifa_engine_last_error()
    assert L.ifa_step_plan_query(0, 0, 0, 0, 1, None) == -1
    rows = (C.c_int * 5)(0, 0, 0, 0, 0)
    pool_rows, out5 = (C.c_int * 1)(), (C.c_int * 5)()
    assert L.ifa_step_plan_batch(0, rows, 1, pool_rows, out5) == 0
    assert L.ifa_step_plan_batch(0, None, 1, pool_rows, out5) == -1
    assert L.ifa_step_plan_batch(0, rows, 0, pool_rows, out5) == -1     # no rows
    assert L.ifa_step_plan_batch(0, rows, 1, None, out5) == -1
    assert L.ifa_step_plan_batch(0, rows, 1, pool_rows, None) == -1
    assert b"ifa_step_plan_batch" in L.ifa_engine_last_error()
    neg = (C.c_int * 5)(0, 1, -1, 0, 0)
    assert L.ifa_step_plan_batch(0, neg, 1, pool_rows, out5) == -1      # a negative pool length
