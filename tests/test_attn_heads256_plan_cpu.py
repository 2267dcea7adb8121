"""CPU-only: the launch plan of prompt attention at head_dim 256 (csrc/ifa_attn_heads256_plan.h) through the host-only entry
ifa_attention_heads256_plan, at the shapes of the device matrix (tests/test_gpu_attn_heads256.py takes SHAPES from here): grid, LDS
bytes, XCD remap; every refusal; ifa_attention_plan still answering Scalar for 256 whatever ifa_attention_mfma_heads says, and
ifa_attention_heads16_plan still refusing 256."""
import ctypes as C

import pytest

import inferflow_amd as ia
from tests import prompt_attn_util as U
from tests.test_attn_heads16_plan_cpu import heads16_plan

F16, Q8 = U.F16, U.Q8
LDS = 2 * 32 * (256 + 8) * 2 + 2 * 256 * (32 + 8) * 2         # [2][32][256 + 8] halfs of K, then [2][256][32 + 8] halfs of V: 74 752


def _sh(heads, kv_heads, kvd, prefix, qt, **k):
    # (kind TwoPass64: prompt_attn_util then probes every 32-key block edge and the group edges of 64-query tiles -- this kernel's staging)
    return U.Shape(U.TWO_PASS64, heads, kv_heads, 256, kvd, prefix, qt, **k)


# queries 4, 5, 31, 32, 33, 127, 128, 129, 257 (a fifth tile of one query; the edges of the 128-query design) behind prefixes 0, 1, 31, 32, 33, 200;
# 8 heads over 1 kv head (Gemma-2B) and over 2, 4 over 4, 6 over 3; 8 heads take the XCD remap; Q8_B32T2 on 10; ALiBi on 2
SHAPES = [
    _sh(8, 1, F16, 0, 4), _sh(6, 3, F16, 1, 5), _sh(8, 2, Q8, 31, 31), _sh(4, 4, F16, 32, 32), _sh(8, 1, F16, 33, 33),
    _sh(8, 2, Q8, 200, 5), _sh(6, 3, F16, 0, 127, alibi=1), _sh(8, 2, F16, 1, 128), _sh(4, 4, Q8, 31, 129), _sh(8, 1, Q8, 32, 33),
    _sh(6, 3, F16, 33, 127), _sh(4, 4, F16, 200, 32), _sh(8, 1, F16, 0, 129), _sh(6, 3, Q8, 1, 129), _sh(4, 4, F16, 33, 257),
    _sh(8, 2, F16, 31, 128, n_ctx=31 + 128 + 40), _sh(8, 1, Q8, 33, 33, n_ctx=33 + 33 + 40),       # more cache rows than the last query may see
    _sh(4, 4, F16, 200, 129, alibi=1), _sh(6, 3, Q8, 32, 4), _sh(4, 4, Q8, 0, 128),
    # the edges of the kernel that was shipped (a wave is 16 queries, a tile 64)
    _sh(8, 1, F16, 1, 15), _sh(8, 2, Q8, 0, 16), _sh(6, 3, F16, 33, 17), _sh(8, 2, F16, 32, 63), _sh(8, 1, Q8, 31, 64), _sh(4, 4, F16, 0, 65),
]
IDS = [s.id.split("-", 1)[1] for s in SHAPES]


def heads256_plan(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, rows_mode=0):
    """ifa_attention_heads256_plan as a dict"""
    facts = (C.c_int * 10)(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, 64, U.NEVER, rows_mode)
    out = (C.c_int * 6)()
    ia.check(ia.lib().ifa_attention_heads256_plan(facts, 10, out, 6))
    return dict(zip(("error", "q_per_wg", "grid_x", "grid_y", "lds", "xcd_remap"), out))


@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_plan_at_the_device_shapes(sh):
    facts = (sh.kvd, sh.n_ctx, sh.qt, sh.prefix, sh.heads, sh.kv_heads, sh.hd)
    p = heads256_plan(*facts)
    assert p == dict(error=0, q_per_wg=64, grid_x=(sh.qt + 63) // 64, grid_y=sh.heads, lds=LDS, xcd_remap=int(sh.heads % 8 == 0)), p
    assert LDS == 74752
    assert heads16_plan(*facts)["error"] == 6          # the 16-wide tile kernel keeps refusing 256
    L = ia.lib()
    prev = L.ifa_attention_mfma_heads(-1)
    try:
        for on in (0, 1):           # the existing plan does not know the switch: 256 is the scalar kernel's
            L.ifa_attention_mfma_heads(on)
            assert sh.plan()["kind"] == U.SCALAR
    finally:
        L.ifa_attention_mfma_heads(prev)


# (kv dtype, n_ctx, q_tokens, prefix, heads, kv_heads, head_dim, rows_mode) -> error
REFUSALS = [
    ((F16, 70, 70, 0, 8, 2, 64, 0), 6), ((F16, 70, 70, 0, 8, 2, 96, 0), 6), ((F16, 70, 70, 0, 8, 8, 128, 0), 6),        # other head sizes
    ((F16, 9, 3, 6, 8, 1, 256, 0), 7), ((Q8, 1, 1, 0, 8, 2, 256, 0), 7),                                               # fewer than 4 queries
    ((F16, 70, 70, 0, 8, 1, 256, 1), 8),                                                                                # the rows entry
    ((U.dt.Q4_B32T1A, 70, 70, 0, 8, 1, 256, 0), 1), ((F16, 70, 70, 0, 8, 3, 256, 0), 2), ((F16, 70, 70, 0, 8, 1, 0, 0), 3),
    ((F16, 0, 70, 0, 8, 1, 256, 0), 4), ((F16, 70, 70, -1, 8, 1, 256, 0), 4), ((F16, 65537, 70, 0, 8, 1, 256, 0), 5), ((F16, 65536, 65536, 0, 16, 16, 256, 0), 5),
]


@pytest.mark.parametrize("facts,error", REFUSALS, ids=["e%d-%d" % (e, i) for i, (_, e) in enumerate(REFUSALS)])
def test_refusals(facts, error):
    p = heads256_plan(*facts)
    assert p == dict(error=error, q_per_wg=0, grid_x=0, grid_y=0, lds=0, xcd_remap=0), p
    if error <= 5:                  # the existing plan's own refusals, unchanged
        assert U.plan(*facts[:7])["error"] == error
