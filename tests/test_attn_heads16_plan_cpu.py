"""CPU-only: the launch plan of k_attention_heads16 (csrc/ifa_attn_heads_plan.h) through the host-only entry ifa_attention_heads16_plan, at
the shapes of the device matrix (tests/test_gpu_attn_heads16.py takes SHAPES from here): grid, LDS bytes, XCD remap; every refusal; and
ifa_attention_plan still answering Scalar for 48 / 80 / 96 whatever ifa_attention_mfma_heads says."""
import ctypes as C

import pytest

import inferflow_amd as ia
from tests import prompt_attn_util as U

F16, Q8 = U.F16, U.Q8
# [2][32][hd + 8] halfs of K, then [2][hd][40] halfs of V
LDS = {48: 2 * 32 * 56 * 2 + 2 * 48 * 40 * 2, 80: 2 * 32 * 88 * 2 + 2 * 80 * 40 * 2, 96: 2 * 32 * 104 * 2 + 2 * 96 * 40 * 2}


def _sh(heads, kv_heads, hd, kvd, prefix, qt, **k):
    # (kind TwoPass64: prompt_attn_util then probes every 32-key block edge and the group edges of 64-query tiles -- this kernel's staging)
    return U.Shape(U.TWO_PASS64, heads, kv_heads, hd, kvd, prefix, qt, **k)


# queries 4, 5, 15, 16, 17 (wave edge), 63, 64, 65 (tile edge), 129 (a partly filled third tile) behind prefixes 0, 1, 31, 32, 33, 200;
# GQA groups 1, 2, 4 (and 3); 8 heads (XCD remap) and 6; Q8_B32T2 at 96, and at 48 / 80 with 2 kv heads (32-blocks straddle the heads)
SHAPES = [
    _sh(8, 2, 48, F16, 0, 4), _sh(6, 6, 48, F16, 1, 5), _sh(8, 4, 48, F16, 31, 15), _sh(8, 2, 48, Q8, 32, 16), _sh(6, 2, 48, F16, 33, 17),
    _sh(8, 8, 48, F16, 200, 63), _sh(8, 2, 48, Q8, 0, 64), _sh(6, 6, 48, F16, 1, 65, alibi=1), _sh(8, 4, 48, F16, 33, 129),
    _sh(8, 2, 48, Q8, 200, 17), _sh(8, 2, 48, F16, 31, 64, n_ctx=31 + 64 + 40),          # more cache rows than the last query may see
    _sh(8, 2, 80, F16, 0, 5), _sh(6, 2, 80, Q8, 1, 4), _sh(8, 4, 80, F16, 32, 15), _sh(8, 8, 80, F16, 33, 16), _sh(8, 2, 80, Q8, 31, 17),
    _sh(6, 6, 80, F16, 0, 63), _sh(8, 2, 80, F16, 200, 64), _sh(8, 2, 80, Q8, 32, 65), _sh(8, 4, 80, F16, 1, 129, alibi=1),
    _sh(6, 2, 80, F16, 200, 5), _sh(8, 2, 80, Q8, 0, 129),
    _sh(8, 8, 96, F16, 0, 4), _sh(6, 3, 96, Q8, 1, 15), _sh(8, 2, 96, F16, 31, 16), _sh(8, 4, 96, Q8, 32, 17), _sh(6, 6, 96, F16, 33, 63),
    _sh(8, 2, 96, Q8, 200, 64), _sh(8, 4, 96, F16, 0, 65), _sh(6, 3, 96, F16, 32, 129), _sh(8, 8, 96, Q8, 33, 65, n_ctx=33 + 65 + 40),
    _sh(8, 2, 96, F16, 1, 5), _sh(8, 4, 96, Q8, 200, 129),
]
IDS = [s.id.split("-", 1)[1] for s in SHAPES]


def heads16_plan(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, rows_mode=0):
    """ifa_attention_heads16_plan as a dict"""
    facts = (C.c_int * 10)(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, 64, U.NEVER, rows_mode)
    out = (C.c_int * 6)()
    ia.check(ia.lib().ifa_attention_heads16_plan(facts, 10, out, 6))
    return dict(zip(("error", "q_per_wg", "grid_x", "grid_y", "lds", "xcd_remap"), out))


@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_plan_at_the_device_shapes(sh):
    p = heads16_plan(sh.kvd, sh.n_ctx, sh.qt, sh.prefix, sh.heads, sh.kv_heads, sh.hd)
    assert p == dict(error=0, q_per_wg=64, grid_x=(sh.qt + 63) // 64, grid_y=sh.heads, lds=LDS[sh.hd], xcd_remap=int(sh.heads % 8 == 0)), p
    L = ia.lib()
    prev = L.ifa_attention_mfma_heads(-1)
    try:
        for on in (0, 1):           # the existing plan does not know the switch: other head sizes are the scalar kernel's
            L.ifa_attention_mfma_heads(on)
            assert L.ifa_attention_mfma_heads(-1) == on
            assert sh.plan()["kind"] == U.SCALAR
    finally:
        L.ifa_attention_mfma_heads(prev)
    assert prev == 0                # the default


# (kv dtype, n_ctx, q_tokens, prefix, heads, kv_heads, head_dim, rows_mode) -> error
REFUSALS = [
    ((F16, 70, 70, 0, 8, 2, 64, 0), 6), ((F16, 70, 70, 0, 8, 2, 128, 0), 6), ((F16, 70, 70, 0, 8, 8, 112, 0), 6),       # other head sizes
    ((F16, 9, 3, 6, 8, 2, 80, 0), 7), ((Q8, 1, 1, 0, 8, 2, 96, 0), 7),                                                # fewer than 4 queries
    ((F16, 70, 70, 0, 8, 2, 80, 1), 8),                                                                                 # the rows entry
    ((U.dt.Q4_B32T1A, 70, 70, 0, 8, 2, 80, 0), 1), ((F16, 70, 70, 0, 8, 3, 80, 0), 2), ((F16, 70, 70, 0, 6, 3, 80, 0), 3),  # 3 x 80: no whole 32-blocks
    ((F16, 0, 70, 0, 8, 2, 80, 0), 4), ((F16, 70, 70, -1, 8, 2, 80, 0), 4), ((F16, 65537, 70, 0, 8, 2, 80, 0), 5), ((F16, 65536, 65536, 0, 8, 2, 96, 0), 5),
]


@pytest.mark.parametrize("facts,error", REFUSALS, ids=["e%d-%d" % (e, i) for i, (_, e) in enumerate(REFUSALS)])
def test_refusals(facts, error):
    p = heads16_plan(*facts)
    assert p == dict(error=error, q_per_wg=0, grid_x=0, grid_y=0, lds=0, xcd_remap=0), p
    if error <= 5:                  # the existing plan's own refusals, unchanged
        assert U.plan(*facts[:7])["error"] == error
