"""-m gpu: nothing of a step's tail survives its call (StepTail, csrc/ifa_engine_state.h; DESIGN.md "Step tails").  One worker runs a
call of every tail kind in one fixed order and in the reverse order, cache and logit state restored between the calls; every result
equals the result the same call gives as the first call of a freshly built worker."""
import numpy as np
import pytest

from inferflow_amd import _capi, dtypes as dt
from inferflow_amd import worker as W
from tests.test_gpu_decode_batch_steps import Bed, mixed_rows

pytestmark = pytest.mark.gpu

K = 8
PARAMS = (4, 0.9, 0.9, 8, 0.05)      # top_p


def _sp(pool):
    return _capi.SampleParams(*PARAMS, pool)


def _plain_decode(b):
    b.wk.select_kv(2)
    return [int(t) for t in b.wk.decode(b.t0[2], b.pos[2], 3, timed=False)[0]]


def _decode_pool_armed(b):
    b.wk.select_kv(1)
    b.wk.pool_adjust([1])
    nxt, ids, vals = b.wk.decode_pool(b.t0[1], b.pos[1], K)
    return nxt, ids.tolist(), vals.tolist()


def _forward_pool(b):
    b.wk.select_kv(0)
    nxt, ids, vals = b.wk.forward_pool(b.prompts[2][:9], 0, K)
    return nxt, ids.tolist(), vals.tolist()


def _forward_score_two_passes(b):
    b.wk.select_kv(0)
    toks = np.concatenate([b.prompts[2], b.prompts[3][:7]]).astype(np.int32)      # 40 tokens: a pass of 32, then one of 8
    assert toks.size == 40
    b.wk.set_option("prefill_mid", 0)      # (this shape has its operand-order copies: 40 tokens would be one pass of the mid kernel)
    try:
        nxt, lse, tl = b.wk.forward_score(toks, 0, np.roll(toks, -1))
        assert b.wk.prompt_route()["first_pass"] == 32, b.wk.prompt_route()      # two passes: the cursor carries the rows of the first
    finally:
        b.wk.set_option("prefill_mid", 1)
    return nxt, lse.tobytes(), tl.tobytes()


def _decode_batch_pool_mixed(b):
    b.wk.pool_adjust([-1, 2])         # rows 0 and 2 pooled, only row 2 armed
    nxt, pools = b.wk.decode_batch_pool(b.t0[:3], b.pos[:3], [0, 1, 2], K, [0, 2])
    return nxt.tolist(), [(i.tolist(), v.tolist()) for i, v in pools]


def _decode_sampled(b):
    b.wk.select_kv(2)
    out, st, _ = b.wk.decode_sampled(b.t0[2], b.pos[2], 3, _sp(50), W.rng_state_of_seed(11), state_slot=2, timed=False)
    return out.tolist(), st


def _decode_draft_sampled(b):
    b.wk.select_kv(1)
    toks = np.concatenate([[b.t0[1]], b.prompts[2][:3]]).astype(np.int32)
    out, st = b.wk.decode_draft_sampled(toks, int(b.pos[1]), _sp(20), W.rng_state_of_seed(12), state_slot=1)
    return out.tolist(), st


def _decode_batch_steps(b):
    out, emitted, states, _ = b.wk.decode_batch_steps(b.t0[:4], b.pos[:4], np.arange(4, dtype=np.int32), 3, mixed_rows(4))
    return out.tolist(), emitted.tolist(), states


CALLS = [_plain_decode, _decode_pool_armed, _forward_pool, _forward_score_two_passes, _decode_batch_pool_mixed, _decode_sampled,
         _decode_draft_sampled, _decode_batch_steps]


def _bed():
    b = Bed("test_gqa", dt.F16, 4)     # 4 KV slots prefilled to 1 / 5 / 33 / 58 keys
    b.arm()
    b.restore()
    return b


def _run(b, call):
    """the call's result and the logit state it leaves (the processed calls count what they emit)"""
    res = call(b)
    b.wk.sync()
    return res, b.state().tobytes()


def test_every_tail_kind_in_both_orders_equals_a_fresh_worker():
    want = {}
    for call in CALLS:
        fresh = _bed()
        try:
            want[call.__name__] = _run(fresh, call)
        finally:
            fresh.wk.close()
    b = _bed()
    try:
        for order in (CALLS, CALLS[::-1]):
            for call in order:
                got = _run(b, call)
                assert got[0] == want[call.__name__][0], (call.__name__, "first" if order is CALLS else "reverse", got[0], want[call.__name__][0])
                assert got[1] == want[call.__name__][1], (call.__name__, "logit state")
                b.restore()
    finally:
        b.wk.close()
