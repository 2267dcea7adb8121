"""CPU-only: the decode route plan (csrc/ifa_decode_route.h, through ifa_decode_route_plan) at head_dim 256, the head size of
k_dec_attn256 / k_dec_attn256_scores (docs/decode_attention_heads256.md).  Expected values written out by hand:
  one workgroup   256 * 6 + 64 + 8 * 256 * 4 + 16 = 9808, + 2 * max_ctx rounded up to 16 (704 keys: 11216)
  P.V of a split  32 + 8 * 256 * 4 + 8208 + 16 = 16448, + 2 * (704 / 8 = 88 rounded up to 64: 128) = 16704
  scores          16 for either cache: the quad mapping reads F16 rows straight into registers, nothing is staged
The plan alone does not keep a 256-wide model off the fused QKV launch: with tail_layers_ok forced to 1 it answers FusedTail.  The
guard is the engine's qkv_attn_layer_ok (dec_qkv_attn_supported refuses every head size but 128), which leaves that fact at 0; it is
tested where it lives, through ifa_model_decode_route in tests/test_gpu_decode_attn_heads256.py."""
import pytest

from tests.test_decode_route_cpu import ONE_WG, SPLIT, TAIL, SMALL, plan, route

GEMMA = dict(SMALL, head_dim=256, heads=8, kv_heads=1, max_ctx=704)


@pytest.mark.parametrize("kv_q8", [0, 1])
@pytest.mark.parametrize("reach", [1, 65, 300])
def test_one_workgroup_route_is_the_256_row_instance_without_a_tile(reach, kv_q8):
    assert plan(GEMMA, reach=reach, kv_q8=kv_q8) == route(ONE_WG, pb=256, kt=0, lds_attn=11216)


@pytest.mark.parametrize("kv_q8", [0, 1])
def test_split_route_needs_no_staging_lds_for_the_scores(kv_q8):
    assert plan(GEMMA, reach=700, kv_q8=kv_q8) == route(SPLIT, nsplits=8, split=8, lds_scores=16, lds_pv=16704)
    assert plan(GEMMA, reach=700, kv_q8=kv_q8, attn_nsplits=32)["lds_pv"] == 16448 + 2 * 64


def test_the_plan_alone_is_not_the_guard_against_the_fused_tail():
    assert plan(GEMMA, reach=65, tail_layers_ok=1, gk=32, rw=3)["kind"] == TAIL


def test_scores_lds_of_the_other_head_sizes_is_unchanged():
    for hd in (32, 48, 64, 80, 96, 128):
        assert plan(GEMMA, head_dim=hd, reach=700)["lds_scores"] == 256 * (2 * hd + 16)
        assert plan(GEMMA, head_dim=hd, reach=700, kv_q8=hd % 32 == 0)["lds_scores"] == (16 if hd % 32 == 0 else 256 * (2 * hd + 16))
