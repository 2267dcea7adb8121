"""No GPU: the service shell with logprobs over the host-only loopback engine (it answers a logprobs query from a fixed table:
candidate j of a step is (next + j) % 1000 with log p = -0.25 - j) -- the fields appear when asked for, in streamed chunks and in the
final message, the body is byte-identical without the request fields, logprobs outside -1..20 are refused -- and the host-side
facts of the new C entries (arguments checked before any HIP call, the split rule a function of (rows, n) only)."""
import ctypes as C
import inspect
import json
import re

import numpy as np

import inferflow_amd as ia
from inferflow_amd import _capi, engine, worker
from tests.logprob_util import bound, lse_f64


def test_new_entries_are_declared_exported_and_bound():
    L = ia.lib()
    for name in ("ifa_logsumexp_rows", "ifa_logsumexp_workspace", "ifa_model_forward_score", "ifa_model_pool_lse"):
        assert name in _capi.SIGNATURES and hasattr(L, name)
    for name in ("ifa_engine_add_query_lp", "ifa_engine_last_logprobs", "ifa_engine_score", "ifa_engine_perplexity_device", "ifa_service_selftest_request"):
        assert name in _capi.ENGINE_SIGNATURES and hasattr(L, name)
    assert "logprobs" in inspect.signature(engine.InferenceEngine.add_query).parameters
    for m in ("last_logprobs", "score"):
        assert hasattr(engine.InferenceEngine, m)
    for m in ("forward_score", "pool_lse", "decode_pool_lse", "forward_pool_lse", "decode_batch_pool_lse"):
        assert hasattr(worker.DecodeWorker, m)
    assert hasattr(worker, "logsumexp_rows")


def test_split_rule_depends_on_rows_and_n_only():
    """workspace bytes = rows * splits * 2 floats; a prompt's many rows take one workgroup each (no workspace), one row of 32000 ids
    is split 16 ways (one 16-byte vector per lane and part), never more than 64 ways, never more than ~128 workgroups in all"""
    ws = ia.lib().ifa_logsumexp_workspace
    assert ws(1, 32000) == 16 * 8 and ws(1, 151936) == 64 * 8 and ws(1, 8) == 0 and ws(1, 2048) == 0 and ws(1, 4096) == 2 * 8
    assert ws(3, 32000) == 3 * 16 * 8 and ws(8, 151936) == 8 * 16 * 8 and ws(63, 151936) == 63 * 2 * 8
    assert ws(64, 151936) == 0 and ws(600, 32000) == 0 and ws(0, 32000) == 0
    for rows in range(1, 64):
        for n in (8, 1000, 32000, 50257, 151936):
            assert ws(rows, n) <= 256 * 4          # (the worker's fixed workspace: rows * splits <= 128 pairs)


def test_arguments_are_checked_before_the_device():
    L = ia.lib()
    buf = np.zeros(64, np.float32); p = buf.ctypes.data_as(C.c_void_p)
    assert L.ifa_logsumexp_rows(None, 64, None, 1, 64, None, p, None, None, None) == -1 and b"null" in L.ifa_last_error()
    assert L.ifa_logsumexp_rows(p, 32, None, 1, 64, None, p, None, None, None) == -1
    assert L.ifa_logsumexp_rows(p, 64, None, 70000, 64, None, p, None, None, None) == -1
    assert L.ifa_logsumexp_rows(p, 64, None, 1, 64, None, p, p, None, None) == -1
    assert L.ifa_model_forward_score(None, p, 1, 0, p, p, p, None) == -1
    assert L.ifa_model_pool_lse(None, p, 1, p) == -1
    toks = (C.c_int * 3)(1, 2, 3)
    assert L.ifa_engine_add_query_lp(None, toks, 3, 0, 0, 1.0, 5) == -1
    assert L.ifa_engine_score(None, toks, 3, buf.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert L.ifa_engine_last_logprobs(None, 1, None, None, None, 0, None) == 0


def test_reference_statement_and_bound():
    row = np.array([1.0, 2.0, 3.0], np.float16)
    assert abs(lse_f64(row) - np.log(np.exp(1.0) + np.exp(2.0) + np.exp(3.0))) < 1e-12
    assert np.isnan(lse_f64(np.array([-np.inf, -np.inf], np.float16))) and np.isnan(lse_f64(np.array([0, np.inf], np.float16)))
    assert np.isnan(lse_f64(np.array([0, np.nan], np.float16))) and lse_f64(np.array([-np.inf, 2.0], np.float16)) == 2.0
    assert bound(2048, 0.5) == 26 * 2.0 ** -24 + 2.0 ** -23 and bound(2049, 10.0) == 28 * 2.0 ** -24 + 10 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the service shell
def _request(body, openai, max_ctx=64):
    buf = C.create_string_buffer(1 << 16)
    rc = ia.lib().ifa_service_selftest_request(json.dumps(body).encode(), int(openai), max_ctx, buf, len(buf))
    assert rc == 0
    return buf.value.decode()


def _format(ids, is_end, openai, chunk, prompt_tokens):
    a = np.asarray(ids, np.int32)
    buf = C.create_string_buffer(1 << 14)
    assert ia.lib().ifa_service_format_response(a.ctypes.data_as(C.POINTER(C.c_int)), len(a), int(is_end), int(openai), int(chunk), prompt_tokens, buf, len(buf)) == 0
    return buf.value.decode()


def _want(ids, n_top):
    return [{"token_id": t, "logprob": -0.25, "top_logprobs": [{"token_id": (t + j) % 1000, "logprob": -0.25 - j} for j in range(n_top)]} for t in ids]


PROMPT_IDS = [5, 6, 7]
GENERATED = [8, 9, 10, 11]


def test_service_emits_logprobs_when_asked_openai_shape():
    for n_top in (0, 3, 20):
        body = {"prompt_token_ids": PROMPT_IDS, "max_tokens": 4, "logprobs": True}
        if n_top:
            body["top_logprobs"] = n_top
        out = json.loads(_request(body, True))
        assert out["ok"] and out["ret_code"] == "succ" and out["chunks"] == []
        choice = out["final"]["choices"][0]
        assert choice["message"]["token_ids"] == GENERATED and choice["finish_reason"] == "length"
        assert choice["logprobs"]["content"] == _want(GENERATED, n_top)
        # streamed: every chunk carries the entries of ITS tokens, the final message all of them
        out = json.loads(_request(dict(body, stream=True), True))
        assert out["ok"]
        seen, entries = [], []
        for ch in out["chunks"]:
            c = ch["choices"][0]
            assert [e["token_id"] for e in c["logprobs"]["content"]] == c["delta"]["token_ids"]
            seen += c["delta"]["token_ids"]; entries += c["logprobs"]["content"]
        assert seen == GENERATED and entries == _want(GENERATED, n_top)
        assert out["final"]["choices"][0]["logprobs"]["content"] == _want(GENERATED, n_top)


def test_service_emits_logprobs_when_asked_native_shape():
    body = {"prompt_token_ids": PROMPT_IDS, "max_output_len": 4, "logprobs": True, "top_logprobs": 2}
    out = json.loads(_request(body, False))
    assert out["ok"] and out["final"]["token_ids"] == GENERATED and out["final"]["logprobs"] == _want(GENERATED, 2)
    out = json.loads(_request(dict(body, is_streaming_mode=True), False))
    got = [e for ch in out["chunks"] for e in ch["logprobs"]]
    assert got == _want(GENERATED, 2) and out["final"]["logprobs"] == _want(GENERATED, 2)


def test_service_body_is_byte_identical_without_the_request_fields():
    """against the formatter as it was (ifa_service_format_response knows nothing of logprobs): final message and streamed chunks"""
    for extra in ({}, {"logprobs": False}):
        raw = _request(dict({"prompt_token_ids": PROMPT_IDS, "max_tokens": 4}, **extra), True)
        assert "logprob" not in raw
        assert raw.endswith('"final": ' + _format(GENERATED, True, True, False, len(PROMPT_IDS)) + "}")
        raw = _request(dict({"prompt_token_ids": PROMPT_IDS, "max_output_len": 4}, **extra), False)
        assert "logprob" not in raw
        want = _format(GENERATED, True, False, False, len(PROMPT_IDS))      # (time_cost is zeroed on both sides)
        assert raw.endswith('"final": ' + want + "}"), (raw, want)
    out = json.loads(_request({"prompt_token_ids": PROMPT_IDS, "max_tokens": 4, "stream": True}, True))
    ids = []
    for ch in out["chunks"]:
        c = ch["choices"][0]
        assert json.dumps(ch) == json.dumps(json.loads(_format(c["delta"]["token_ids"], c["finish_reason"] is not None, True, True, len(PROMPT_IDS))))
        assert "logprobs" not in c
        ids += c["delta"]["token_ids"]
    assert ids == GENERATED
    # the parser's echo of a request without the fields is unchanged; with them it names the count
    buf = C.create_string_buffer(4096)
    assert ia.lib().ifa_service_parse_request(json.dumps({"prompt_token_ids": [1, 2]}).encode(), 0, buf, len(buf)) == 0
    assert "logprobs" not in buf.value.decode()
    assert ia.lib().ifa_service_parse_request(json.dumps({"prompt_token_ids": [1, 2], "logprobs": True, "top_logprobs": 7}).encode(), 0, buf, len(buf)) == 0
    assert json.loads(buf.value.decode())["logprobs"] == 7
    assert ia.lib().ifa_service_parse_request(json.dumps({"prompt_token_ids": [1, 2], "logprobs": True}).encode(), 1, buf, len(buf)) == 0
    assert json.loads(buf.value.decode())["logprobs"] == 0


def test_logprobs_outside_the_range_are_rejected():
    buf = C.create_string_buffer(4096)
    for openai in (0, 1):
        for bad in ({"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1}, {"logprobs": True, "top_logprobs": 1000},
                    {"top_logprobs": 3}, {"logprobs": False, "top_logprobs": 3}, {"logprobs": "yes"}, {"logprobs": True, "top_logprobs": "5"}):
            body = dict({"prompt_token_ids": [1, 2]}, **bad)
            assert ia.lib().ifa_service_parse_request(json.dumps(body).encode(), openai, buf, len(buf)) == -1, bad
            assert "error.invalid_logprobs" in buf.value.decode()
            out = json.loads(_request(body, openai))
            assert not out["ok"] and out["ret_code"] == "error.invalid_logprobs" and out["final"] is None
        for good in (0, 1, 20):
            assert ia.lib().ifa_service_parse_request(json.dumps({"prompt_token_ids": [1, 2], "logprobs": True, "top_logprobs": good}).encode(), openai, buf, len(buf)) == 0
