"""The prompt prefix cache's reuse policy (inferflow_amd/host/prefix_cache.h) through its host-only entry point
ifa_prefix_cache_plan: which slot a new query takes, how many leading rows it reuses, and whether they are copied."""
import ctypes as C

import inferflow_amd as ia
from inferflow_amd.engine import prefix_cache_plan as plan

S = list(range(100, 140))               # a 40-token shared prefix
P = S + [7, 8, 9]                       # the new prompt


def test_empty_records_give_the_lowest_free_slot():
    assert plan([[], [], []], [0, 0, 0], [0, 0, 0], P) == (0, -1, 0)
    assert plan([[], [], []], [1, 0, 0], [5, 0, 0], P) == (1, -1, 0)
    assert plan([[], [], []], [1, 1, 0], [5, 6, 0], P) == (2, -1, 0)


def test_record_equal_to_the_prompt_is_capped_one_short():
    assert plan([[], list(P)], [0, 0], [0, 3], P) == (1, -1, len(P) - 1)
    # a record LONGER than the prompt too: one token must run to produce logits
    assert plan([list(P) + [1, 2, 3]], [0], [1], P) == (0, -1, len(P) - 1)
    # a one-token prompt can reuse nothing
    assert plan([[5]], [0], [1], [5], min_tokens=1) == (0, -1, 0)


def test_min_tokens_threshold():
    rec = S[:15] + [1, 1, 1]
    assert plan([[], rec], [0, 0], [0, 1], P, min_tokens=16) == (0, -1, 0)
    assert plan([[], S[:16] + [1, 1]], [0, 0], [0, 1], P, min_tokens=16) == (1, -1, 16)
    assert plan([[], S[:1] + [1]], [0, 0], [0, 1], P, min_tokens=1) == (1, -1, 1)
    # below the threshold with no empty record around: the oldest free slot is overwritten, even if it is the short match
    assert plan([rec, [3, 3, 3]], [0, 0], [1, 2], P, min_tokens=16) == (0, -1, 0)


def test_best_match_on_a_busy_slot_is_copied_to_a_free_one():
    # a free slot with an empty record goes before an OLDER non-empty one
    assert plan([list(S), [9, 9], []], [1, 0, 0], [10, 1, 20], P) == (2, 0, 40)
    # among non-empty ones the oldest stamp wins (lower index among equal stamps)
    assert plan([list(S), [9, 9], [8, 8], [7]], [1, 0, 0, 0], [10, 5, 3, 4], P) == (2, 0, 40)
    assert plan([list(S), [9, 9], [8, 8]], [1, 0, 0], [10, 3, 3], P) == (1, 0, 40)
    # the destination is never the source, whatever the stamps say
    assert plan([[4], list(S)], [0, 1], [9, 0], P) == (0, 1, 40)
    for src in range(3):
        recs = [[1], [2], [3]]; busy = [0, 0, 0]
        recs[src] = list(S); busy[src] = 1
        slot, s, n = plan(recs, busy, [0, 0, 0], P)
        assert s == src and slot != src and n == 40


def test_equal_match_prefers_the_free_slot_in_place():
    assert plan([list(S), list(S) + [1]], [1, 0], [1, 2], P) == (1, -1, 40)
    assert plan([list(S) + [1], list(S)], [0, 1], [1, 2], P) == (0, -1, 40)
    # two free slots with the same match: the lower index
    assert plan([[], list(S), list(S)], [0, 0, 0], [0, 9, 1], P) == (1, -1, 40)


def test_longer_match_on_a_busy_slot_beats_a_shorter_free_one():
    assert plan([S[:30], list(S), []], [0, 1, 0], [1, 2, 0], P) == (2, 1, 40)
    # ... and with no empty record the shorter free match is what gets overwritten
    assert plan([S[:30], list(S)], [0, 1], [1, 2], P) == (0, 1, 40)
    # a longer free match wins over a shorter busy one, in place
    assert plan([list(S), S[:30]], [0, 1], [1, 2], P) == (0, -1, 40)


def test_bad_arguments_return_minus_one():
    L = ia.lib()
    one = (C.c_int * 1)(0)
    st = (C.c_longlong * 1)(0)
    pr = (C.c_int * 3)(1, 2, 3)
    out = (C.c_int * 3)()
    assert L.ifa_prefix_cache_plan(None, one, one, st, 1, pr, 3, 16, out) == 0          # (no records at all is fine)
    assert L.ifa_prefix_cache_plan(None, one, one, st, 0, pr, 3, 16, out) == -1         # no slots
    assert L.ifa_prefix_cache_plan(None, one, one, st, 1, pr, 0, 16, out) == -1         # empty prompt
    assert L.ifa_prefix_cache_plan(None, one, one, st, 1, None, 3, 16, out) == -1
    assert L.ifa_prefix_cache_plan(None, one, one, st, 1, pr, 3, 0, out) == -1          # min_tokens < 1
    assert L.ifa_prefix_cache_plan(None, one, one, st, 1, pr, 3, 16, None) == -1
    assert L.ifa_prefix_cache_plan(None, None, one, st, 1, pr, 3, 16, out) == -1
    neg = (C.c_int * 1)(-1)
    assert L.ifa_prefix_cache_plan(None, neg, one, st, 1, pr, 3, 16, out) == -1         # negative record length
    two = (C.c_int * 1)(2)
    assert L.ifa_prefix_cache_plan(None, two, one, st, 1, pr, 3, 16, out) == -1         # a record without its tokens
    assert b"ifa_prefix_cache_plan" in L.ifa_engine_last_error()
    assert plan([[1], [2]], [1, 1], [0, 0], P) is None                                  # every slot busy
