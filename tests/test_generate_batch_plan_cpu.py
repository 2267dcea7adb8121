"""The round rule of InferenceEngine::GenerateBatch in pure code (host/step_plan.h PlanGenerateBatch, ifa_generate_batch_plan): no
device, no engine."""
import ctypes as C

import inferflow_amd as ia

GREEDY, PROCESSED, DRAWN = 0, 1, 2
DONE, FED, SINGLE = 0, 1, 2
NONE, DUPLICATE, MULTI_GPU, TENSORS, TOO_MANY, NEEDS_SAMPLER, NO_ROOM, BAD_ARGUMENT = range(8)


def q(id, remaining, room=1000, shift=0, kind=GREEDY, stops=0):
    return (id, remaining, room, shift, kind, stops)


def plan(queries, min_queries=2, round_steps=32, fused_max=32, sampler=1, multi=0, tensors=0):
    facts = [min_queries, round_steps, fused_max, sampler, multi, tensors, len(queries)] + [int(v) for qq in queries for v in qq]
    out = (C.c_int * (4 + 2 * len(queries)))(*([-9] * (4 + 2 * len(queries))))
    assert ia.lib().ifa_generate_batch_plan((C.c_int * len(facts))(*facts), len(facts), out, len(out)) == 0
    m = out[3]
    return dict(refusal=out[0], refused_id=out[1], route=out[2], rounds=[(out[4 + 2 * i], out[5 + 2 * i]) for i in range(m)])


def test_round_length_is_the_minimum_of_cap_remaining_and_room():
    assert plan([q(1, 100), q(2, 50)])["rounds"] == [(1, 32), (2, 32)]                     # the cap
    assert plan([q(1, 100), q(2, 5)])["rounds"] == [(1, 5), (2, 5)]                       # a query's budget: it leaves at a round boundary
    assert plan([q(1, 100, room=100), q(2, 50, room=3, shift=1)])["rounds"] == [(1, 3), (2, 3)]      # a shift-on query's room
    assert plan([q(1, 7, room=7), q(2, 9, room=20)], round_steps=256)["rounds"] == [(1, 7), (2, 7)]
    assert plan([q(1, 100), q(2, 50)], round_steps=1)["rounds"] == [(1, 1), (2, 1)]
    p = plan([q(1, 100), q(2, 50)])
    assert (p["refusal"], p["route"]) == (NONE, FED)


def test_ascending_id_order_and_finished_queries_left_out():
    p = plan([q(9, 10), q(3, 0), q(5, 4), q(1, 8)])
    assert p["route"] == FED and p["rounds"] == [(1, 4), (5, 4), (9, 4)]
    assert plan([q(4, 0), q(2, 0)]) == dict(refusal=NONE, refused_id=0, route=DONE, rounds=[])
    assert plan([])["route"] == DONE


def test_under_the_threshold_each_query_runs_alone():
    assert plan([q(7, 20)]) == dict(refusal=NONE, refused_id=0, route=SINGLE, rounds=[(7, 20)])
    assert plan([q(7, 20), q(8, 0)])["route"] == SINGLE
    p = plan([q(3, 20), q(1, 9, kind=DRAWN), q(2, 5, kind=PROCESSED)], min_queries=4)
    assert p["route"] == SINGLE and p["rounds"] == [(1, 9), (2, 5), (3, 20)]
    assert plan([q(1, 20), q(2, 20)], min_queries=1)["route"] == FED                       # never a batch of one: the threshold is at least 2
    assert plan([q(1, 20)], min_queries=1)["route"] == SINGLE
    # more rows than a fused step takes do not matter where nothing is batched
    assert plan([q(1, 20), q(2, 20), q(3, 20)], min_queries=4, fused_max=2)["route"] == SINGLE


def test_stop_ids_under_the_threshold():
    # a greedy query is trimmed on the host: a chunk of at most the round cap, inside its room
    assert plan([q(1, 100, stops=1)])["rounds"] == [(1, 32)]
    assert plan([q(1, 100, room=6, shift=1, stops=1)])["rounds"] == [(1, 6)]
    assert plan([q(1, 10, stops=1)])["rounds"] == [(1, 10)]
    # a drawn or processed one steps one token at a time, so that generator and counts stay exact
    assert plan([q(1, 100, kind=DRAWN, stops=1)])["rounds"] == [(1, 1)]
    assert plan([q(1, 100, kind=PROCESSED, stops=1)])["rounds"] == [(1, 1)]
    assert plan([q(1, 100, kind=DRAWN)])["rounds"] == [(1, 100)]
    # in a batched round the stop ids are tested on the device: nothing changes
    assert plan([q(1, 100, kind=DRAWN, stops=1), q(2, 100, stops=1)])["rounds"] == [(1, 32), (2, 32)]


def test_every_refusal_plans_nothing():
    def refused(p, why, id=0):
        assert p == dict(refusal=why, refused_id=id, route=DONE, rounds=[]), p
    two = [q(1, 10), q(2, 10)]
    refused(plan(two, multi=1), MULTI_GPU)
    refused(plan(two, tensors=1), TENSORS)
    refused(plan(two, round_steps=0), BAD_ARGUMENT)
    refused(plan(two, round_steps=257), BAD_ARGUMENT)
    refused(plan([q(1, 10), q(2, -1)]), BAD_ARGUMENT, 2)
    refused(plan([q(1, 10), q(2, 10), q(1, 3)]), DUPLICATE, 1)
    refused(plan([q(1, 10), q(2, 10, kind=DRAWN)], sampler=0), NEEDS_SAMPLER, 2)
    refused(plan([q(1, 10), q(2, 10, kind=PROCESSED)], sampler=0), NEEDS_SAMPLER, 2)
    refused(plan([q(1, 10), q(2, 10, room=9)]), NO_ROOM, 2)                                # no shift: the budget must fit
    assert plan([q(1, 10), q(2, 10, room=9, shift=1)])["rounds"] == [(1, 9), (2, 9)]       # with the shift the round ends at the limit
    refused(plan([q(1, 10), q(2, 10, room=0, shift=1)]), NO_ROOM, 1)                       # at the limit with nothing dropped
    refused(plan([q(i, 10) for i in range(1, 18)], fused_max=16), TOO_MANY)
    assert plan([q(i, 10) for i in range(1, 17)], fused_max=16)["route"] == FED
    refused(plan([q(i, 10 if i < 17 else 0) for i in range(1, 18)] + [q(99, 5)], fused_max=16), TOO_MANY)      # 17 live of 18
    refused(plan([q(1, 10), q(2, 10)], fused_max=0), TOO_MANY)


def test_bad_arguments_are_codes():
    L = ia.lib()
    out = (C.c_int * 8)()
    assert L.ifa_generate_batch_plan(None, 7, out, 8) == -1
    f = (C.c_int * 13)(2, 32, 32, 1, 0, 0, 1, 1, 10, 100, 0, 3, 0)                         # kind 3
    assert L.ifa_generate_batch_plan(f, 13, out, 8) == -1
    f[11] = 0
    assert L.ifa_generate_batch_plan(f, 12, out, 8) == -1                                   # the count does not match n
    assert L.ifa_generate_batch_plan(f, 13, out, 5) == -1                                   # no room for the answer
    assert L.ifa_generate_batch_plan(f, 13, out, 8) == 0 and list(out[:6]) == [0, 0, SINGLE, 1, 1, 10]
