"""The feed rule compiled for the host (ifa_batch_feed_host, csrc/ifa_batch_feed.h) against the numpy restatement of its
specification (tests/batch_feed_util.py), byte for byte after every step; then each edge of the rule spelled out on the big case,
so that a mistake shared by the two would still show."""
import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import worker as W
from inferflow_amd._capi import BatchFeedArgs
from tests import batch_feed_util as U

CASES = U.cases()


def _run_host(n, layers, A, inputs, check_each_step=True):
    want = U.clone(A)
    for s, inp in enumerate(inputs):
        U.load_inputs(A, inp)
        U.load_inputs(want, inp)
        W.batch_feed_host(n, layers, A)
        U.feed_ref(n, layers, want)
        if check_each_step:
            U.assert_same(A, want, "step %d" % s)
    return A


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_rule_equals_numpy(case):
    _, n, layers, A, inputs = case
    _run_host(n, layers, U.clone(A), inputs)


def test_every_edge_of_the_rule_on_32_rows_and_80_layers():
    _, n, layers, A0, inputs = CASES[0]
    A = _run_host(n, layers, U.clone(A0), inputs, check_each_step=False)
    steps = len(inputs)
    rows, ring = A["rows"], A["ring"]
    tok = lambda s, r: U.token_of(A0["rows"], inputs[s], r)
    rng = lambda s, r: inputs[s]["rng"][A0["rows"]["sel"][r]]
    assert int(A["step"][0]) == steps
    # stops at step 0, in the middle, on the last step, on the 8th of 8 stop ids: emitted counts the stop id, the ring holds it, -1 behind
    for r, at in ((0, 0), (1, 2), (2, steps - 1), (3, 3)):
        assert rows["live"][r] == 0 and rows["emitted"][r] == at + 1
        assert [int(x) for x in ring[:, r]] == [tok(s, r) for s in range(at + 1)] + [-1] * (steps - 1 - at)
        # frozen: the row keeps the token and position it had when it stopped, in every layer
        assert A["pos"][r] == A0["pos"][r] + at and A["tok"][r] == (tok(at - 1, r) if at else A0["tok"][r])
        assert (A["attn_rows"]["n_ctx"][:, r] == A0["attn_rows"]["n_ctx"][:, r] + at).all()
        # the generator word behind the row's LAST OWN draw, though rng[r] moved on every later step
        # (a plain greedy row has no generator: its word is left alone)
        if A0["rows"]["kind"][r] == U.ARGMAX:
            assert rows["rng_final"][r] == A0["rows"]["rng_final"][r]
        else:
            assert rows["rng_final"][r] == rng(at, r) and (at == steps - 1 or rng(at + 1, r) != rng(at, r))
    # rows that never stop: 8 ids without a hit, none, other rows' tokens, an id behind n_stop
    for r in (4, 5, 10, 12):
        assert rows["live"][r] == 1 and rows["emitted"][r] == steps and A["pos"][r] == A0["pos"][r] + steps
        assert [int(x) for x in ring[:, r]] == [tok(s, r) for s in range(steps)] and A["tok"][r] == tok(steps - 1, r)
        assert (A["attn_rows"]["n_ctx"][:, r] == A0["attn_rows"]["n_ctx"][:, r] + steps).all()
    # frozen before the call: nothing but ring = -1 (and the pair switched off)
    assert (ring[:, 6] == -1).all() and A["pair_slot"][6] == -1
    assert rows[6:7].tobytes() == A0["rows"][6:7].tobytes() and A["tok"][6] == A0["tok"][6] and A["pos"][6] == A0["pos"][6]
    assert (A["attn_rows"]["n_ctx"][:, 6] == A0["attn_rows"]["n_ctx"][:, 6]).all()
    # undrawable rows: the first failure in (step, row) order owns the word -- row 8 of step 1, not row 13 of step 1, not row 20 of step 3
    assert int(A["err"][0]) == 1 + 1 * n + 8
    for r, at in ((8, 1), (13, 1), (20, 3)):
        assert rows["live"][r] == 0 and rows["emitted"][r] == at and (ring[at:, r] == -1).all() and A["pos"][r] == A0["pos"][r] + at
    # the pairs of the last step: (state slot, token) of every row that emitted, slot -1 for the others
    for r in range(n):
        if ring[steps - 1, r] >= 0:
            assert (A["pair_slot"][r], A["pair_tok"][r]) == (A0["rows"]["state_slot"][r], ring[steps - 1, r])
        else:
            assert A["pair_slot"][r] == -1
    # the cache pointers of the table are nobody's to touch
    assert A["attn_rows"]["kc"].tobytes() == A0["attn_rows"]["kc"].tobytes() and A["attn_rows"]["vc"].tobytes() == A0["attn_rows"]["vc"].tobytes()


def test_struct_layouts_match_the_header():
    import ctypes as C
    assert W.BATCH_FEED_ROW.itemsize == 64 and W.BATCH_ATTN_ROW.itemsize == 24 and W.BATCH_ATTN_ROW.fields["n_ctx"][1] == 16
    assert C.sizeof(BatchFeedArgs) == 24 + 14 * 8


def test_argument_refusals():
    L = ia.lib()
    _, n, layers, A, inputs = CASES[1]
    A = U.clone(A)
    a = W._batch_feed_args(n, layers, A, lambda v: v.ctypes.data)
    import ctypes as C
    for field, value, word in (("struct_size", 8, b"struct_size"), ("n", 0, b"n 0"), ("n", 33, b"n 33"), ("layers", -1, b"layers"),
                               ("ring_steps", 0, b"ring_steps"), ("ring_steps", 257, b"ring_steps"), ("tok", None, b"null"),
                               ("attn_rows", None, b"attention table"), ("pool_counts", None, b"come together"), ("k_stride", 0, b"k_stride")):
        keep = getattr(a, field)
        setattr(a, field, value)
        before = U.clone(A)
        assert L.ifa_batch_feed_host(C.byref(a)) == -1 and word in L.ifa_last_error(), field
        assert L.ifa_batch_feed_rows(C.byref(a), None) == -1 and word in L.ifa_last_error(), field      # refused before any device call
        U.assert_same(A, before, field)
        setattr(a, field, keep)
    assert L.ifa_batch_feed_host(C.byref(a)) == 0
    assert L.ifa_batch_clamp_counts(None, None, 1, None) == -1 and b"null" in L.ifa_last_error()
