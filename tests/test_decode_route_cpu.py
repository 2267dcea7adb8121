"""CPU-only checks of the decode route plan (csrc/ifa_decode_route.h) through the host-only entry point ifa_decode_route_plan: which
attention launch a decode step runs, with which kernel instance (entry bucket pb, K tile kt, unloaded heads ul), how many splits, which
chained FFN launch and how much dynamic LDS.  Tables only; the expected values are written out by hand from rules R1 - R10 of DESIGN.md
("Decode route plan"), not computed.

LDS bytes used below (nsplit = 256 // (head_dim // 8)):
  one workgroup / fused tail  head_dim * 6 + 64 + nsplit * head_dim * 4 + 16 + tile rows * head_dim * 2 + 2 * max_ctx rounded up to 16
                              = 8464 / 8432 / 8656 / 8560 / 8720 / 9040 for head_dim 32 / 48 / 64 / 80 / 96 / 128, + tile + score row
  P.V of a split              32 + nsplit * head_dim * 4 + 8208 + 16 + 2 * (max_ctx / nsplits rounded up, then up to 64)
                              = 16448 for head_dim 32 / 64 / 128, 16320 for 48 / 96, 16256 for 80, + the probabilities
  scores of a split           256 * (2 * head_dim + 16) for an F16 cache, 16 for a Q8 cache"""
import ctypes as C

import pytest

import inferflow_amd as ia
from inferflow_amd import _capi

ONE_WG, SPLIT, TAIL = 0, 1, 2
LDS = 160 * 1024
FACTS = ("head_dim", "heads", "kv_heads", "max_ctx", "kv_q8", "reach", "attn_split_ctx", "attn_nsplits", "attn_kt", "attn_unload", "fuse_attn",
         "fuse_ffn", "attn_q8", "tail_layers_ok", "gk", "rw", "chain_level", "have_attq", "waits", "num_cus", "visible_cus", "own_launches")
OUT = ("kind", "nsplits", "pb", "kt", "ul", "gk", "rw", "chain", "split_threshold", "split", "lds_attn", "lds_scores", "lds_pv", "error")

# Llama-2-7B on 256 CUs: 32 / 32 heads of 128, every layer takes the fused launch with 8 workgroups per kv group, 6 rows per wave
LLAMA = dict(head_dim=128, heads=32, kv_heads=32, max_ctx=4096, kv_q8=0, reach=1, attn_split_ctx=-1, attn_nsplits=0, attn_kt=1, attn_unload=1,
             fuse_attn=1, fuse_ffn=0, attn_q8=1, tail_layers_ok=1, gk=8, rw=6, chain_level=2, have_attq=1, waits=1, num_cus=256, visible_cus=256,
             own_launches=0)
GQA = dict(LLAMA, kv_heads=8, gk=32, rw=3)                                        # grouped queries (Mixtral-8x7B's attention)
SMALL = dict(LLAMA, max_ctx=640, tail_layers_ok=0, gk=0, rw=0, chain_level=0)     # the one-layer test models: no fused launch


def facts_of(base, **over):
    f = dict(base)
    f.update(over)
    assert set(f) == set(FACTS)
    return f


def plan(base, **over):
    f = facts_of(base, **over)
    facts = (C.c_int * len(FACTS))(*[int(f[k]) for k in FACTS])
    out = (C.c_int * len(OUT))(*([-7] * len(OUT)))
    assert ia.lib().ifa_decode_route_plan(facts, len(FACTS), out, len(OUT)) == 0
    return dict(zip(OUT, out))


def route(kind, pb=0, kt=0, ul=0, nsplits=0, gk=0, rw=0, chain=0, thr=320, split=0, lds_attn=0, lds_scores=0, lds_pv=0, error=0):
    return dict(kind=kind, nsplits=nsplits, pb=pb, kt=kt, ul=ul, gk=gk, rw=rw, chain=chain, split_threshold=thr, split=split,
                lds_attn=lds_attn, lds_scores=lds_scores, lds_pv=lds_pv, error=error)


def tail7b(pb, kt=1, ul=0, lds_attn=0, thr=512, **more):
    return route(TAIL, pb=pb, kt=kt, ul=ul, gk=8, rw=6, thr=thr, lds_attn=lds_attn, **more)


TABLE = [
    # ---- Llama-2-7B at the bucket and split edges (R3, R4, R6, R9): 64 / 128 rows through the K tile, 256 with unloaded heads
    ("7b-64", facts_of(LLAMA, reach=64), tail7b(64, lds_attn=33616)),
    ("7b-65", facts_of(LLAMA, reach=65), tail7b(128, lds_attn=50000)),
    ("7b-128", facts_of(LLAMA, reach=128), tail7b(128, lds_attn=50000)),
    ("7b-129", facts_of(LLAMA, reach=129), tail7b(256, ul=1, lds_attn=82768)),
    ("7b-512", facts_of(LLAMA, reach=512), tail7b(256, ul=1, lds_attn=82768)),
    ("7b-513", facts_of(LLAMA, reach=513), route(SPLIT, nsplits=8, thr=512, split=8, lds_scores=69632, lds_pv=17472)),
    ("7b-8192", facts_of(LLAMA, max_ctx=16384, reach=8192), route(SPLIT, nsplits=8, thr=512, split=8, lds_scores=69632, lds_pv=20544)),
    ("7b-8193", facts_of(LLAMA, max_ctx=16384, reach=8193), route(SPLIT, nsplits=16, thr=512, split=16, lds_scores=69632, lds_pv=18496)),
    # ---- grouped queries: the threshold is 640 (R2)
    ("gqa-640", facts_of(GQA, reach=640), route(TAIL, pb=256, kt=1, ul=1, gk=32, rw=3, thr=640, lds_attn=82768)),
    ("gqa-641", facts_of(GQA, reach=641), route(SPLIT, nsplits=8, thr=640, split=8, lds_scores=69632, lds_pv=17472)),
    # ---- a fused-launch geometry without UL kernels (16 / 16 heads: 16 workgroups per kv group, 3 rows per wave): the loaded-heads
    # kernel runs, and the threshold is still the 512 measured for the UL kernels -- ADVICE r6 item 5, kept as it is on purpose
    ("no-ul-shape", facts_of(LLAMA, heads=16, kv_heads=16, gk=16, rw=3, reach=300), route(TAIL, pb=256, kt=1, ul=0, gk=16, rw=3, thr=512, lds_attn=82768)),
    ("no-ul-shape-513", facts_of(LLAMA, heads=16, kv_heads=16, gk=16, rw=3, reach=513), route(SPLIT, nsplits=8, thr=512, split=8, lds_scores=69632, lds_pv=17472)),
    # ---- half the CUs visible: the fused launch's grid cannot be resident (R1), nor the chained launch's (R10)
    ("cus128-300", facts_of(LLAMA, visible_cus=128, fuse_ffn=2, reach=300), route(ONE_WG, pb=256, kt=1, lds_attn=82768)),
    ("cus128-321", facts_of(LLAMA, visible_cus=128, fuse_ffn=2, reach=321), route(SPLIT, nsplits=8, split=8, lds_scores=69632, lds_pv=17472)),
    # ---- no waiting launches
    ("waits0", facts_of(LLAMA, waits=0, fuse_ffn=2, reach=100), route(ONE_WG, pb=128, kt=1, lds_attn=50000)),
    ("fuse_attn0", facts_of(LLAMA, fuse_attn=0, fuse_ffn=2, reach=100), route(ONE_WG, pb=128, kt=1, chain=2, lds_attn=50000)),
    # ---- the tensor-parallel step: its own launches, the threshold as without it
    ("own-400", facts_of(LLAMA, own_launches=1, fuse_ffn=2, reach=400), route(ONE_WG, pb=256, kt=1, thr=512, lds_attn=82768)),
    ("own-513", facts_of(LLAMA, own_launches=1, reach=513), route(SPLIT, nsplits=8, thr=512, split=8, lds_scores=69632, lds_pv=17472)),
    # ---- attn_split_ctx: 0 never, else from that many keys on
    ("ctx0", facts_of(LLAMA, attn_split_ctx=0, reach=4000), tail7b(256, ul=1, lds_attn=82768, thr=0)),
    ("ctx1-1", facts_of(LLAMA, attn_split_ctx=1, reach=1), tail7b(64, lds_attn=33616, thr=1)),
    ("ctx1-2", facts_of(LLAMA, attn_split_ctx=1, reach=2), route(SPLIT, nsplits=8, thr=1, split=8, lds_scores=69632, lds_pv=17472)),
    ("ctx320-320", facts_of(LLAMA, attn_split_ctx=320, reach=320), tail7b(256, ul=1, lds_attn=82768, thr=320)),
    ("ctx320-321", facts_of(LLAMA, attn_split_ctx=320, reach=321), route(SPLIT, nsplits=8, thr=320, split=8, lds_scores=69632, lds_pv=17472)),
    # ---- attn_nsplits replaces the count, capped at 32 (R7)
    ("nsplits16", facts_of(LLAMA, attn_nsplits=16, reach=513), route(SPLIT, nsplits=16, thr=512, split=8, lds_scores=69632, lds_pv=16960)),
    ("nsplits64", facts_of(LLAMA, attn_nsplits=64, reach=513), route(SPLIT, nsplits=32, thr=512, split=8, lds_scores=69632, lds_pv=16704)),
    ("nsplits16-q8", facts_of(LLAMA, kv_q8=1, attn_nsplits=16, reach=513), route(SPLIT, nsplits=16, thr=512, split=8, lds_scores=16, lds_pv=16960)),
    # ---- head sizes without the bucketed instances (R8): always 256 rows, no K tile
    ("hd48", facts_of(SMALL, head_dim=48, reach=65), route(ONE_WG, pb=256, lds_attn=9712)),
    ("hd80", facts_of(SMALL, head_dim=80, reach=65), route(ONE_WG, pb=256, lds_attn=9840)),
    ("hd96", facts_of(SMALL, head_dim=96, reach=65), route(ONE_WG, pb=256, lds_attn=10000)),
    ("hd96-q8", facts_of(SMALL, head_dim=96, kv_q8=1, reach=64), route(ONE_WG, pb=256, lds_attn=10000)),
    ("hd64", facts_of(SMALL, head_dim=64, reach=65), route(ONE_WG, pb=128, kt=1, lds_attn=26320)),
    ("hd64-kt0", facts_of(SMALL, head_dim=64, attn_kt=0, reach=65), route(ONE_WG, pb=128, lds_attn=9936)),
    ("hd32-q8", facts_of(SMALL, head_dim=32, kv_q8=1, reach=64), route(ONE_WG, pb=64, lds_attn=9744)),
    # ---- the score row against the LDS (R5): head_dim 64 holds 8656 + 2 * max_ctx <= 163840, i.e. 77592 keys; one more forces the
    # split from position 0 on (split = 0).  At 77592 the K tile no longer fits (R8)
    ("lds-77592", facts_of(SMALL, head_dim=64, max_ctx=77592, reach=100), route(ONE_WG, pb=128, kt=0, lds_attn=163840)),
    ("lds-77593", facts_of(SMALL, head_dim=64, max_ctx=77593, reach=100), route(SPLIT, nsplits=8, lds_scores=36864, lds_pv=35904)),
    ("lds-81920-q8", facts_of(SMALL, head_dim=64, max_ctx=81920, kv_q8=1, reach=700), route(SPLIT, nsplits=8, split=8, lds_scores=16, lds_pv=36928)),
    # ---- R7 doubles: 8 splits of 600000 keys need 16448 + 2 * 75008 = 166464 bytes, 16 splits 16448 + 2 * 37504
    ("lds-doubles", facts_of(SMALL, head_dim=64, max_ctx=600000, reach=100), route(SPLIT, nsplits=16, lds_scores=36864, lds_pv=91456)),
    # ---- R7 gives up: 32 splits of 2400000 keys still need 166464 bytes
    ("lds-error", facts_of(SMALL, head_dim=64, max_ctx=2400000, reach=100), route(SPLIT, nsplits=32, lds_scores=36864, lds_pv=166464, error=1)),
    ("lds-error-nsplits", facts_of(SMALL, head_dim=64, max_ctx=600000, attn_nsplits=8, reach=100), route(SPLIT, nsplits=8, lds_scores=36864, lds_pv=166464, error=1)),
    # ---- the chained FFN launch (R10)
    ("ffn0", facts_of(LLAMA, fuse_ffn=0, reach=100), tail7b(128, lds_attn=50000, chain=0)),
    ("ffn1", facts_of(LLAMA, fuse_ffn=1, reach=100), tail7b(128, lds_attn=50000, chain=1)),
    ("ffn1-no-attq", facts_of(LLAMA, fuse_ffn=1, have_attq=0, reach=100), tail7b(128, lds_attn=50000, chain=1)),
    ("ffn2", facts_of(LLAMA, fuse_ffn=2, reach=100), tail7b(128, lds_attn=50000, chain=2)),
    ("ffn3", facts_of(LLAMA, fuse_ffn=3, reach=100), tail7b(128, lds_attn=50000, chain=2)),
    ("ffn2-no-attq", facts_of(LLAMA, fuse_ffn=2, have_attq=0, reach=100), tail7b(128, lds_attn=50000, chain=1)),
    ("ffn2-attn_q8-0", facts_of(LLAMA, fuse_ffn=2, attn_q8=0, reach=100), tail7b(128, lds_attn=50000, chain=1)),
    ("ffn2-level1", facts_of(LLAMA, fuse_ffn=2, chain_level=1, reach=100), tail7b(128, lds_attn=50000, chain=1)),
    ("ffn2-level0", facts_of(LLAMA, fuse_ffn=2, chain_level=0, reach=100), tail7b(128, lds_attn=50000, chain=0)),
    ("ffn2-split", facts_of(LLAMA, fuse_ffn=2, reach=513), route(SPLIT, nsplits=8, chain=2, thr=512, split=8, lds_scores=69632, lds_pv=17472)),
    ("ffn2-hd48", facts_of(SMALL, head_dim=48, fuse_ffn=2, chain_level=2, reach=65), route(ONE_WG, pb=256, chain=1, lds_attn=9712)),
]


@pytest.mark.parametrize("name,facts,want", TABLE, ids=[t[0] for t in TABLE])
def test_route_table(name, facts, want):
    assert plan(facts) == want


# attn_unload x entry bucket x cache format on the Llama-2-7B shape: the EFFECTIVE (pb, kt, ul) of the launched instance (R9).
# reach 64 / 128 / 200 are the 64 / 128 / 256-row buckets (200: attn_unload 0 lowers the threshold to 320).  F16 without the K tile
# has the 256-row instance only; unloaded heads exist for 256 rows, and with attn_unload 2 for 128 rows through the K tile or Q8.
F16_KT, F16_NO_KT, Q8 = dict(attn_kt=1, kv_q8=0), dict(attn_kt=0, kv_q8=0), dict(attn_kt=1, kv_q8=1)
UNLOAD = {
    (0, "f16-kt"): [(64, 1, 0), (128, 1, 0), (256, 1, 0)],
    (0, "f16-no-kt"): [(256, 0, 0), (256, 0, 0), (256, 0, 0)],
    (0, "q8"): [(64, 0, 0), (128, 0, 0), (256, 0, 0)],
    (1, "f16-kt"): [(64, 1, 0), (128, 1, 0), (256, 1, 1)],
    (1, "f16-no-kt"): [(256, 0, 0), (256, 0, 0), (256, 0, 1)],
    (1, "q8"): [(64, 0, 0), (128, 0, 0), (256, 0, 1)],
    (2, "f16-kt"): [(64, 1, 0), (128, 1, 1), (256, 1, 1)],
    (2, "f16-no-kt"): [(256, 0, 0), (256, 0, 0), (256, 0, 1)],
    (2, "q8"): [(64, 0, 0), (128, 0, 1), (256, 0, 1)],
}
FMT = {"f16-kt": F16_KT, "f16-no-kt": F16_NO_KT, "q8": Q8}
KT_LDS = {64: 33616, 128: 50000, 256: 82768}      # 17232 + pb * 256


@pytest.mark.parametrize("unload,fmt", sorted(UNLOAD), ids=["unload%d-%s" % k for k in sorted(UNLOAD)])
def test_unload_buckets_and_formats(unload, fmt):
    for reach, (pb, kt, ul) in zip((64, 128, 200), UNLOAD[(unload, fmt)]):
        got = plan(LLAMA, attn_unload=unload, reach=reach, **FMT[fmt])
        want = tail7b(pb, kt=kt, ul=ul, lds_attn=KT_LDS[pb] if kt else 17232, thr=512 if unload else 320)
        assert got == want, (unload, fmt, reach)


def test_lds_formulas_on_the_edge_matrix():
    """dec_attn_smem / dec_attn_pv_smem / dec_attn_scores_smem on the shapes of tests/test_gpu_decode_attn_edges.py (head_dim, max_ctx):
    the numbers the formulas gave before they moved into ifa_decode_route.h"""
    one_wg = {(32, 640): 9744, (48, 640): 9712, (64, 640): 9936, (80, 640): 9840, (96, 640): 10000, (128, 640): 10320, (64, 320): 9296}
    for (hd, ctx), want in one_wg.items():      # no K tile: attn_kt 0
        assert plan(SMALL, head_dim=hd, max_ctx=ctx, attn_kt=0, reach=300)["lds_attn"] == want, (hd, ctx)
    tiles = {(32, 64): 13840, (32, 128): 17936, (32, 256): 26128, (64, 64): 18128, (64, 128): 26320, (64, 256): 42704,
             (128, 64): 26704, (128, 128): 43088, (128, 256): 75856}
    for (hd, pb), want in tiles.items():        # max_ctx 640 with a tile of pb rows
        assert plan(SMALL, head_dim=hd, reach={64: 64, 128: 128, 256: 300}[pb])["lds_attn"] == want, (hd, pb)
    for hd, scores in ((64, 36864), (128, 69632)):      # the split walks: max_ctx 704, 8 / 16 / 32 splits
        for nsp, pv in ((8, 16704), (16, 16576), (32, 16576)):
            r = plan(SMALL, head_dim=hd, max_ctx=704, attn_split_ctx=1, attn_nsplits=nsp, reach=700)
            assert (r["kind"], r["nsplits"], r["lds_scores"], r["lds_pv"]) == (SPLIT, nsp, scores, pv), (hd, nsp)
        assert plan(SMALL, head_dim=hd, max_ctx=704, kv_q8=1, attn_split_ctx=1, reach=700)["lds_scores"] == 16
    assert plan(SMALL, head_dim=64, max_ctx=320, attn_split_ctx=1, reach=300)["lds_pv"] == 16576      # the ALiBi variant's split walk
    assert plan(SMALL, head_dim=32, max_ctx=640, attn_split_ctx=1, reach=300)["lds_scores"] == 20480


def test_bad_arguments_are_refused():
    facts = (C.c_int * len(FACTS))(*[int(LLAMA[k]) for k in FACTS])
    out = (C.c_int * len(OUT))()
    L = ia.lib()
    assert L.ifa_decode_route_plan(facts, len(FACTS) - 1, out, len(OUT)) != 0
    assert L.ifa_decode_route_plan(facts, len(FACTS), out, len(OUT) - 1) != 0
    assert L.ifa_decode_route_plan(None, len(FACTS), out, len(OUT)) != 0
    facts[0] = 0                                # head_dim
    assert L.ifa_decode_route_plan(facts, len(FACTS), out, len(OUT)) != 0


def test_symbols_exported_and_bound():
    for name in ("ifa_decode_route_plan", "ifa_model_decode_route"):
        assert hasattr(ia.lib(), name), "missing symbol " + name
        assert name in _capi.SIGNATURES
