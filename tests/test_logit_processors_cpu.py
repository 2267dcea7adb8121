"""CPU: the service shell's view of the logit processors (repetition_penalty, presence_penalty, frequency_penalty, logit_bias) --
the request parser accepts them in both shapes, echoes them only when given and refuses what is out of range -- and the new
entry points are exported and bound."""
import ctypes as C
import json

import pytest

import inferflow_amd as ia
from inferflow_amd import _capi


def _parse(body, openai=False):
    out = C.create_string_buffer(1 << 16)
    rc = ia.lib().ifa_service_parse_request(json.dumps(body).encode(), int(openai), out, len(out))
    return rc, json.loads(out.value.decode())


def _body(openai, **extra):
    b = {"messages": [{"role": "user", "content_token_ids": [1, 2, 3]}]} if openai else {"prompt_token_ids": [1, 2, 3]}
    b.update(extra)
    return b


@pytest.mark.parametrize("openai", [False, True])
def test_parser_accepts_and_echoes_the_four_fields(openai):
    rc, js = _parse(_body(openai, repetition_penalty=1.3, presence_penalty=-2, frequency_penalty=0.5,
                          logit_bias={"7": -100, "999": 5.25, "0": 100}), openai)
    assert rc == 0, js
    assert js["prompt_token_ids"] == [1, 2, 3]
    assert js["repetition_penalty"] == pytest.approx(1.3) and js["presence_penalty"] == -2.0 and js["frequency_penalty"] == 0.5
    assert js["logit_bias"] == {"7": -100.0, "999": 5.25, "0": 100.0}
    # one field alone: only that one is echoed
    rc, js = _parse(_body(openai, frequency_penalty=2), openai)
    assert rc == 0 and js["frequency_penalty"] == 2.0
    assert not {"repetition_penalty", "presence_penalty", "logit_bias"} & set(js)
    rc, js = _parse(_body(openai, logit_bias={}), openai)
    assert rc == 0 and js["logit_bias"] == {}


@pytest.mark.parametrize("openai", [False, True])
def test_parser_echo_is_unchanged_without_the_fields(openai):
    rc, js = _parse(_body(openai, temperature=0.5), openai)
    assert rc == 0
    assert not {"repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"} & set(js)
    assert sorted(js) == sorted(["prompt_token_ids", "max_output_len", "decoding_alg", "random_seed", "temperature", "is_streaming_mode",
                                 "eos_token_id", "fn"])


@pytest.mark.parametrize("openai", [False, True])
@pytest.mark.parametrize("field,value", [("presence_penalty", 2.5), ("presence_penalty", -2.01), ("frequency_penalty", 3), ("frequency_penalty", -2.5),
                                         ("repetition_penalty", 0), ("repetition_penalty", -1.0), ("repetition_penalty", "1.2"),
                                         ("presence_penalty", [1]), ("frequency_penalty", None)])
def test_parser_rejects_an_out_of_range_penalty(openai, field, value):
    rc, js = _parse(_body(openai, **{field: value}), openai)
    assert rc == -1 and js == {"ret_code": "error.invalid_penalty"}


@pytest.mark.parametrize("openai", [False, True])
@pytest.mark.parametrize("bias", [
    {"5": "high"},                                  # a non-numeric bias
    {"5": None},
    {"5": 101},                                     # a value of 101
    {"5": -100.5},
    {str(i): 1 for i in range(301)},                # 301 entries
    {"five": 1}, {"5.5": 1}, {"-3": 1}, {"": 1}, {" 5": 1},      # a non-integer key
    [5, 1], 3,                                      # not an object
])
def test_parser_rejects_a_bad_logit_bias(openai, bias):
    rc, js = _parse(_body(openai, logit_bias=bias), openai)
    assert rc == -1 and js == {"ret_code": "error.invalid_logit_bias"}


def test_parser_takes_300_entries_and_the_range_ends():
    rc, js = _parse(_body(False, logit_bias={str(i): (-100 if i % 2 else 100) for i in range(300)}, presence_penalty=2, frequency_penalty=-2))
    assert rc == 0 and len(js["logit_bias"]) == 300 and js["logit_bias"]["1"] == -100.0 and js["logit_bias"]["0"] == 100.0


def test_an_engine_without_processors_answers_unsupported():
    """the service loop over the loopback engine (no logit processors): a processed request ends with error.unsupported, the same
    request without the fields runs"""
    out = C.create_string_buffer(1 << 16)
    for extra, code in (({"presence_penalty": 1.0}, "error.unsupported"), ({"logit_bias": {"3": -5}}, "error.unsupported"),
                        ({"repetition_penalty": 1.0, "presence_penalty": 0, "logit_bias": {}}, "succ"), ({}, "succ")):
        body = dict(prompt_token_ids=[1, 2, 3], max_output_len=2, **extra)
        assert ia.lib().ifa_service_selftest_request(json.dumps(body).encode(), 0, 32, out, len(out)) == 0
        assert json.loads(out.value.decode())["ret_code"] == code, (extra, out.value)


def test_every_new_symbol_is_exported_and_bound():
    L = ia.lib()
    for name in ("ifa_logit_adjust_rows", "ifa_logit_state_reset", "ifa_logit_state_add", "ifa_model_logit_state_reset",
                 "ifa_model_logit_state_add", "ifa_model_pool_adjust"):
        assert name in _capi.SIGNATURES and hasattr(L, name), name
    assert "ifa_engine_add_query_opt" in _capi.ENGINE_SIGNATURES and hasattr(L, "ifa_engine_add_query_opt")
    # the struct the C header declares: a leading struct_size, then the fields in the header's order
    names = [f[0] for f in _capi.QueryOptions._fields_]
    assert names[0] == "struct_size" and names[1:] == ["strategy_id", "random_seed", "temperature", "logprobs", "repetition_penalty",
                                                       "presence_penalty", "frequency_penalty", "n_logit_bias", "logit_bias_ids", "logit_bias_values"]
    # argument checks come before any device call
    assert L.ifa_logit_adjust_rows(None, 8, None, None, 1, 8, None, None, None, None, None) == -1 and b"null" in L.ifa_last_error()
    assert L.ifa_engine_add_query_opt(None, None, 0, None) == -1
