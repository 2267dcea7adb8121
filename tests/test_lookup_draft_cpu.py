"""CPU-only checks of ifa_lookup_draft (host/lookup_draft.h): the rule that picks the draft tokens of lookup decoding."""
import ctypes as C

import pytest

import inferflow_amd as ia
from inferflow_amd import _capi


def draft(ctx, pred, ngram_max=3, ngram_min=1, k=4):
    L = ia.lib()
    a = (C.c_int * max(1, len(ctx)))(*ctx)
    p = (C.c_int * max(1, len(pred)))(*pred) if pred else None
    out = (C.c_int * max(1, k))(*([-7] * max(1, k)))
    n = L.ifa_lookup_draft(a, len(ctx), p, len(pred), ngram_max, ngram_min, k, out)
    if n < 0:
        return n
    assert 0 <= n <= k
    assert all(out[i] == -7 for i in range(n, k)), "nothing is written past the draft"
    return [out[i] for i in range(n)]


def test_symbols_exported_and_bound():
    L = ia.lib()
    for name in ("ifa_lookup_draft", "ifa_engine_generate_lookup", "ifa_model_decode_draft"):
        assert hasattr(L, name), "missing symbol " + name
    assert "ifa_lookup_draft" in _capi.ENGINE_SIGNATURES and "ifa_engine_generate_lookup" in _capi.ENGINE_SIGNATURES
    assert "ifa_model_decode_draft" in _capi.SIGNATURES


def test_longest_ngram_first():
    # the last token (5) continues with 9 after [.. 5]; the last three tokens [3, 4, 5] continue with 7, 8
    ctx = [5, 9, 1, 3, 4, 5, 7, 8, 2, 3, 4, 5]
    assert draft(ctx, [], k=2) == [7, 8]
    # with ngram_max = 1 only the single-token key counts: the only earlier 5 is at index 0
    assert draft([5, 9, 1, 3, 4, 6, 7, 8, 2, 3, 4, 5], [], ngram_max=1, k=2) == [9, 1]
    # a longer key without a match falls through to a shorter one
    assert draft([1, 2, 9, 9, 3, 2], [], k=3) == [9, 9, 3]


def test_prediction_before_context():
    ctx = [1, 2, 3, 50, 60, 1, 2, 3]
    assert draft(ctx, [], k=2) == [50, 60]
    assert draft(ctx, [9, 1, 2, 3, 70, 80], k=2) == [70, 80]
    # the prediction wins at the SAME g only: a 3-gram match in the context beats a 1-gram match in the prediction
    assert draft(ctx, [3, 70, 80], k=2) == [50, 60]
    # ... and a longer match in the prediction beats nothing: g = 3 fails in both, g = 2 hits the prediction before the context
    assert draft([7, 2, 3, 50, 8, 2, 3], [2, 3, 70], k=2) == [70]


def test_lowest_start_in_prediction_highest_in_context():
    assert draft([4, 5], [4, 5, 10, 11, 4, 5, 20, 21], ngram_max=2, k=2) == [10, 11]
    assert draft([4, 5, 10, 11, 4, 5, 20, 21, 4, 5], [], ngram_max=2, k=2) == [20, 21]


def test_cut_at_k_and_at_the_end_of_the_source():
    pred = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert draft([0, 1, 2], pred, k=4) == [3, 4, 5, 6]
    assert draft([0, 1, 2], pred, k=1) == [3]
    assert draft([0, 1, 2], pred, k=7) == [3, 4, 5, 6, 7, 8, 9]
    assert draft([0, 6, 7, 8], pred, k=7) == [9]
    # context source: the continuation ends at the end of the context
    assert draft([1, 2, 3, 9, 1, 2, 3], [], k=7) == [9, 1, 2, 3]


def test_match_with_empty_continuation_is_skipped():
    # [7, 8, 9] ends the prediction: nothing follows it there, so the earlier context match serves (same g)
    assert draft([7, 8, 9, 40, 7, 8, 9], [1, 7, 8, 9], k=2) == [40, 7]
    # the context key itself (start n_ctx - g) is no match: no other occurrence, shorter keys neither
    assert draft([1, 2, 3], [], k=2) == []
    # prediction's only match is at its very end and the context has none: falls to g = 1, where pred [.. 9] also ends -> context
    assert draft([9, 5, 8, 9], [8, 9], ngram_max=2, k=2) == [5, 8]


def test_context_shorter_than_the_key():
    assert draft([3], [1, 2, 3, 4], ngram_max=3, k=2) == [4]            # g = 3, 2 skipped (n_ctx < g), g = 1 matches
    assert draft([2, 3], [1, 2, 3, 4], ngram_max=3, k=2) == [4]         # g = 2
    assert draft([], [1, 2, 3], k=2) == []
    assert draft([3], [1, 2, 3, 4], ngram_max=3, ngram_min=2, k=2) == []


def test_empty_prediction_and_no_match():
    assert draft([1, 2, 3, 4], [], k=3) == []
    assert draft([1, 2, 3, 4], [5, 6, 7], k=3) == []
    assert draft([1, 2, 1], [], k=3) == [2, 1]


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=-1), dict(ngram_min=0), dict(ngram_max=1, ngram_min=2)])
def test_bad_arguments(kw):
    assert draft([1, 2, 3], [1, 2, 3, 4], **kw) == -1


def test_null_pointers_and_negative_lengths():
    L = ia.lib()
    a = (C.c_int * 4)(1, 2, 3, 4)
    out = (C.c_int * 4)()
    assert L.ifa_lookup_draft(None, 4, a, 4, 3, 1, 4, out) == -1
    assert L.ifa_lookup_draft(a, 4, a, 4, 3, 1, 4, None) == -1
    assert L.ifa_lookup_draft(a, 4, None, 4, 3, 1, 4, out) == -1       # a prediction length without a prediction
    assert L.ifa_lookup_draft(a, -1, a, 4, 3, 1, 4, out) == -1
    assert L.ifa_lookup_draft(a, 4, a, -1, 3, 1, 4, out) == -1
    assert L.ifa_lookup_draft(a, 4, None, 0, 3, 1, 4, out) == 0        # no prediction at all is fine
