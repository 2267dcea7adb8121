"""Host-only checks of the context shift: the policy (ifa_context_shift_plan), the service's two request fields, and the numpy model
of the device arithmetic (tests/kv_shift_util.py) against an fp64 rotation -- the guard of the rotation's direction."""
import ctypes as C
import json

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd.engine import context_shift_plan as plan
from tests import kv_shift_util as ku


# ---------------------------------------------------------------------------------------------- the plan
def test_no_shift_below_the_limit():
    for ctx in (8, 64, 1024):
        for n in (1, 2, ctx // 2, ctx - 1):
            for keep in (0, 4, ctx // 2):
                assert plan(n, max(n - 1, 0), ctx, keep) == (), (n, ctx, keep)
                assert plan(n, n, ctx, keep) == ()


@pytest.mark.parametrize("ctx", [8, 64, 65, 320, 1024])
def test_plan_at_the_limit(ctx):
    for keep in (0, 4, ctx // 2):
        processed = ctx - 1                                 # the last committed token has not run
        got = plan(ctx, processed, ctx, keep)
        assert got == (keep, max(1, (processed - keep + 1) // 2)), (ctx, keep, got)
    assert plan(64, 63, 64, 4) == (4, 30) and plan(64, 63, 64, 0) == (0, 32) and plan(64, 63, 64, 32) == (32, 16)


def test_discard_is_at_least_one_and_the_moved_rows_never_outnumber_the_dropped_ones():
    for ctx in (2, 3, 8, 9, 64, 65, 127):
        for keep in range(0, ctx // 2 + 1):
            for processed in range(0, ctx + 1):
                got = plan(ctx, processed, ctx, keep)
                assert got is not None, (ctx, keep, processed)
                if processed <= keep:
                    assert got == ()                          # nothing behind the kept rows is in the cache: nothing to drop
                    continue
                k, d = got
                assert k == keep and d >= 1 and k + d <= processed
                assert processed - k - d <= d, (ctx, keep, processed, d)      # one launch with disjoint source and destination
                assert ctx - d < ctx                                          # the query has room again


def test_bad_arguments():
    for args in ((65, 63, 64, 4), (64, 65, 64, 4), (64, 63, 64, 33), (64, 63, 64, -1), (-1, 0, 64, 4), (10, -1, 64, 4), (1, 0, 1, 0), (0, 0, 0, 0)):
        assert plan(*args) is None, args
    assert ia.lib().ifa_context_shift_plan(64, 63, 64, 4, None) == -1


# ---------------------------------------------------------------------------------------------- the service's request fields
def _parse(body, openai=False):
    buf = C.create_string_buffer(1 << 16)
    rc = ia.lib().ifa_service_parse_request(body.encode(), int(openai), buf, len(buf))
    return rc, json.loads(buf.value.decode())


def _request(body, openai=False, max_ctx=32):
    buf = C.create_string_buffer(1 << 18)
    assert ia.lib().ifa_service_selftest_request(body.encode(), int(openai), max_ctx, buf, len(buf)) == 0
    return json.loads(buf.value.decode())


def test_parser_round_trips_the_two_fields():
    rc, r = _parse('{"prompt_token_ids": [1, 2, 3], "context_shift": true, "context_keep": 7}')
    assert rc == 0 and r["context_shift"] is True and r["context_keep"] == 7
    rc, r = _parse('{"prompt_token_ids": [1, 2, 3], "context_shift": false}')
    assert rc == 0 and r["context_shift"] is False and "context_keep" not in r
    rc, r = _parse('{"messages": [{"content_token_ids": [4, 5]}], "context_keep": 0}', openai=True)
    assert rc == 0 and r["context_keep"] == 0 and "context_shift" not in r
    rc, r = _parse('{"prompt_token_ids": [1, 2, 3]}')
    assert rc == 0 and "context_shift" not in r and "context_keep" not in r
    rc, r = _parse('{"prompt_token_ids": [1, 2, 3], "context_shift": 1}')          # (a number reads as a bool, like "logprobs")
    assert rc == 0 and r["context_shift"] is True
    for bad in ('"context_shift": "yes"', '"context_keep": -1', '"context_keep": 1.5', '"context_keep": true'):
        rc, r = _parse('{"prompt_token_ids": [1, 2, 3], %s}' % bad)
        assert rc == -1 and r["ret_code"] == "error.invalid_context_shift", bad


def test_an_engine_that_cannot_shift_answers_unsupported():
    r = _request('{"prompt_token_ids": [1, 2, 3], "max_output_len": 4, "context_shift": true}')
    assert r["ok"] is False and r["ret_code"] == "error.unsupported"
    r = _request('{"prompt_token_ids": [1, 2, 3], "max_output_len": 4, "context_shift": false, "context_keep": 2}')
    assert r["ok"] is True and r["final"]["token_ids"] == [4, 5, 6, 7]
    # the loopback engine keeps ShiftsContext() == false: a long request is still cut at the room behind the prompt
    r = _request('{"prompt_token_ids": [1, 2, 3], "max_output_len": 100}', max_ctx=16)
    assert r["ok"] is True and len(r["final"]["token_ids"]) == 13


# ---------------------------------------------------------------------------------------------- the numpy model against fp64
def _rot64(k, pos, head_dim, rope_order, theta=10000.0):
    """R(pos) k in fp64 for one head row k [head_dim], full rotary"""
    out = k.copy()
    for c, i0, i1 in ku.pairs(head_dim, rope_order, head_dim):
        a = pos * theta ** (-2.0 * c / head_dim)
        out[i0] = k[i0] * np.cos(a) - k[i1] * np.sin(a)
        out[i1] = k[i0] * np.sin(a) + k[i1] * np.cos(a)
    return out


@pytest.mark.parametrize("rope_order", [1, 2])
def test_model_rotates_back_by_discard_positions(rope_order):
    """model(f16(R(p) k)) lies within 2^-9 * ||pair||_2 of R(p - d) k per element: two F16 roundings of at most 2^-11 relative each
    plus the fp32 angle error (below 3e-5 at positions up to 300) come to under 2^-10; the bound carries a factor 2 of margin.  With
    the rotation the wrong way round the error is of the order of the pair's norm."""
    rng = np.random.default_rng(5)
    hd = 64
    worst = 0.0
    for _ in range(40):
        p = int(rng.integers(1, 301))
        d = int(rng.integers(1, min(p, 299) + 1))
        k = rng.normal(0, 1, hd)
        stored = _rot64(k, p, hd, rope_order).astype(np.float16)
        table = ku.shift_table(hd, hd, d)
        got = ku.rotate_halves(stored[None, :], table, hd, rope_order, hd)[0].astype(np.float64)
        want = _rot64(k, p - d, hd, rope_order)
        wrong = _rot64(k, p + d, hd, rope_order)
        for c, i0, i1 in ku.pairs(hd, rope_order, hd):
            norm = np.hypot(k[i0], k[i1])
            for i in (i0, i1):
                worst = max(worst, abs(got[i] - want[i]) / norm)
                assert abs(got[i] - want[i]) <= 2.0 ** -9 * norm, (p, d, i, got[i], want[i], norm)
        far = max(abs(got[i] - wrong[i]) / np.hypot(k[i0], k[i1]) for c, i0, i1 in ku.pairs(hd, rope_order, hd) for i in (i0, i1))
        assert far > 2.0 ** -9, (p, d)                       # (the check can tell the two directions apart)
    print("worst |error| / ||pair||: %.3g (bound %.3g)" % (worst, 2.0 ** -9))


def test_model_q8_round_trip_and_verbatim_blocks():
    """the Q8 path: an identity table leaves a row's values where dequantise -> quantise leaves them, and with partial rotary the
    blocks without a rotated column keep their bytes although requantising is not idempotent"""
    rng = np.random.default_rng(9)
    kv_heads, hd = 2, 64
    rows = ku.q8_quant(rng.normal(0, 1, (5, kv_heads, hd // 32, 32)).astype(np.float16)).reshape(5, -1)
    assert rows.shape[1] == ku.row_bytes(ku.Q8, kv_heads, hd) == 136
    ident = np.tile(np.asarray([[1.0, 0.0]], np.float32), (hd // 2, 1))
    same = ku.rotate_rows(rows, ku.Q8, kv_heads, hd, 2, hd, ident)
    want = ku.q8_quant(ku.q8_dequant(rows.reshape(5, kv_heads, 2, 34))).reshape(5, -1)
    assert np.array_equal(same, want)
    table = ku.unit_table(hd, rng)
    part = ku.rotate_rows(rows, ku.Q8, kv_heads, hd, 2, 32, table).reshape(5, kv_heads, 2, 34)
    assert np.array_equal(part[:, :, 1], rows.reshape(5, kv_heads, 2, 34)[:, :, 1])
    assert not np.array_equal(part[:, :, 0], rows.reshape(5, kv_heads, 2, 34)[:, :, 0])
    k2, v2 = ku.shift(rows.reshape(-1), rows.reshape(-1).copy(), ku.Q8, kv_heads, hd, 0, 0, None, 1, 2, 5)
    assert np.array_equal(k2, v2) and np.array_equal(v2[136:3 * 136], rows.reshape(-1)[3 * 136:]) and np.array_equal(v2[3 * 136:], rows.reshape(-1)[3 * 136:])
