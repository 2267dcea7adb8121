"""CPU-only checks of the prompt and batched-step route plans (csrc/ifa_prompt_route.h) through the host-only entry points
ifa_prompt_route_plan / ifa_batch_route_plan: which kernels the linears of a layer go through, from which copy of the weights, what is
built first, two passes or one.  Tables only; the expected values are written out by hand from rules P1 - P12 and B1 - B5 of DESIGN.md
("Prompt route plan"), not computed."""
import ctypes as C

import pytest

from inferflow_amd import _capi

EXACT, OPS, ROWS, MID, BIG = 0, 1, 2, 3, 4
K_ROWS, K_MID, K_BIG = 0, 1, 2
TILED, MO, X32 = 0, 1, 2
FACTS = ("T", "exact_order", "perf_stat", "prefill_chunk", "prefill_mid", "prefill_mid_max", "prefill_big", "prefill_big_min", "prefill_res_mid",
         "rows_mo", "gemm_rows", "batch_fused", "gemm_splitk", "rows_kparts", "topo", "experts", "rows_layers", "big_layers", "mid_shapes")
PRODUCTS = ("qkv", "wo", "w13", "w2")
OUT = ("kind", "first_pass", "norm_fused", "res_mid") + tuple(p + "_" + k for p in PRODUCTS for k in ("kernel", "src", "mo", "no_waits")) + (
    "need_mo", "need_x32")
B_FACTS = ("n", "exact_order", "may_chunk", "rows_mo", "gemm_rows", "batch_fused", "rows_kparts", "batch_graph", "graph", "topo", "rows_layers",
           "has_moe", "logits_out")
B_OUT = ("kind", "chunk", "norm_fused", "captured", "gm_kernel", "gm_src", "gm_mo", "gm_no_waits", "need_mo")
B_EXACT, B_OPS, B_FUSED = 0, 1, 2

# a dense Q4_B32T1A model of Llama-2-7B width at the default options: every route is open to it
DENSE = dict(T=1, exact_order=0, perf_stat=0, prefill_chunk=1, prefill_mid=1, prefill_mid_max=768, prefill_big=1, prefill_big_min=47,
             prefill_res_mid=2048, rows_mo=1, gemm_rows=1, batch_fused=1, gemm_splitk=1, rows_kparts=1, topo=0, experts=0, rows_layers=2,
             big_layers=1, mid_shapes=1)
B64 = dict(DENSE, rows_layers=1)                     # a 64-weight nibble format: the rows GEMM only from MO copies
MOE = dict(DENSE, experts=8, mid_shapes=0)           # device-routed experts: no dense FFN matrices
B_DENSE = dict(n=2, exact_order=0, may_chunk=1, rows_mo=1, gemm_rows=1, batch_fused=1, rows_kparts=1, batch_graph=0, graph=1, topo=0,
               rows_layers=2, has_moe=0, logits_out=0)


def _call(fn, names, outs, f):
    assert set(f) == set(names)
    facts = (C.c_int * len(names))(*[int(f[k]) for k in names])
    out = (C.c_int * len(outs))(*([-7] * len(outs)))
    assert fn(facts, len(names), out, len(outs)) == 0
    return dict(zip(outs, out))


def plan(base, **over):
    import inferflow_amd as ia
    return _call(ia.lib().ifa_prompt_route_plan, FACTS, OUT, dict(base, **over))


def bplan(base, **over):
    import inferflow_amd as ia
    return _call(ia.lib().ifa_batch_route_plan, B_FACTS, B_OUT, dict(base, **over))


def route(kind, gm=(0, 0, 0, 0), res=None, first_pass=0, norm_fused=0, need_mo=0, need_x32=0):
    """gm: (kernel, src, mo, no_waits) of the four products; res: that of wo / w2 where it differs (res_mid)"""
    r = dict(kind=kind, first_pass=first_pass, norm_fused=norm_fused, res_mid=1 if res else 0, need_mo=need_mo, need_x32=need_x32)
    for p in PRODUCTS:
        g = res if res and p in ("wo", "w2") else gm
        r.update({p + "_kernel": g[0], p + "_src": g[1], p + "_mo": g[2], p + "_no_waits": g[3]})
    return r


def ops(need_mo=0):
    return route(OPS, need_mo=need_mo)


def rows_mo(norm_fused, first_pass=0, need_mo=1, no_waits=0):
    return route(ROWS, (K_ROWS, MO, 1, no_waits), norm_fused=norm_fused, first_pass=first_pass, need_mo=need_mo)


def rows_tiled(norm_fused, first_pass=0, need_mo=1):
    return route(ROWS, (K_ROWS, TILED, 0, 0), norm_fused=norm_fused, first_pass=first_pass, need_mo=need_mo)


def mid(no_waits=0):
    return route(MID, (K_MID, MO, 1, no_waits), need_mo=1)


def big(need_mo=0, res=False, no_waits=0, res_no_waits=0):
    return route(BIG, (K_BIG, X32, 0, no_waits), res=(K_MID, MO, 1, res_no_waits) if res else None, need_mo=need_mo, need_x32=1)


TABLE = [
    # ---- the lengths at the default options: one row (P10: never the rows GEMM), the norm prologue up to 16 rows with MO copies (P11),
    # the rows GEMM to 32, k_gemm_mid from 33 to prefill_mid_max (P6; 34..48: one pass, P3), above it the large tiles with wo / w2
    # through k_gemm_mid up to prefill_res_mid (P7 - P9: the MO copies are built AFTER the x32 copies, need_mo 2)
    ("T1", dict(DENSE, T=1), ops()),
    ("T2", dict(DENSE, T=2), rows_mo(1)),
    ("T8", dict(DENSE, T=8), rows_mo(1)),
    ("T9", dict(DENSE, T=9), rows_mo(1)),
    ("T16", dict(DENSE, T=16), rows_mo(1)),
    ("T17", dict(DENSE, T=17), rows_mo(0)),
    ("T32", dict(DENSE, T=32), rows_mo(0)),
    ("T33", dict(DENSE, T=33), mid()),
    ("T34", dict(DENSE, T=34), mid()),
    ("T48", dict(DENSE, T=48), mid()),
    ("T49", dict(DENSE, T=49), mid()),
    ("T768", dict(DENSE, T=768), mid()),
    ("T769", dict(DENSE, T=769), big(need_mo=2, res=True)),
    ("T2048", dict(DENSE, T=2048), big(need_mo=2, res=True)),
    ("T2049", dict(DENSE, T=2049), big()),
    # ---- without MO copies (rows_mo 0): the norm prologue to 8 rows only (P11), the rows GEMM to 16 (P4), nothing of k_gemm_mid (P2);
    # 34..48 tokens: no pass of 32 rows, so one pass (P3): op by op up to prefill_big_min, large tiles above it
    ("mo0-T2", dict(DENSE, rows_mo=0, T=2), rows_tiled(1)),
    ("mo0-T8", dict(DENSE, rows_mo=0, T=8), rows_tiled(1)),
    ("mo0-T9", dict(DENSE, rows_mo=0, T=9), rows_tiled(0)),
    ("mo0-T16", dict(DENSE, rows_mo=0, T=16), rows_tiled(0)),
    ("mo0-T17", dict(DENSE, rows_mo=0, T=17), ops()),
    ("mo0-T32", dict(DENSE, rows_mo=0, T=32), ops()),
    ("mo0-T40", dict(DENSE, rows_mo=0, T=40), ops()),
    ("mo0-T48", dict(DENSE, rows_mo=0, T=48), big()),
    ("mo0-T769", dict(DENSE, rows_mo=0, T=769), big()),
    # the re-plan after ensure_mo switched the option off: a 20-token prompt planned on the rows GEMM goes op by op
    ("downgrade-T20-before", dict(DENSE, rows_mo=1, T=20), rows_mo(0)),
    ("downgrade-T20-after", dict(DENSE, rows_mo=0, T=20), ops()),
    # ---- prefill_mid 0: two passes for 34..48 tokens (P3; the first pass's route is shown, each pass builds its own copies: need_mo 0),
    # 33 and 49 in one pass; prefill_big_min 47: 47 / 48 in two passes, with prefill_chunk 0 op by op / large tiles
    ("mid0-T33", dict(DENSE, prefill_mid=0, T=33), ops()),
    ("mid0-T34", dict(DENSE, prefill_mid=0, T=34), rows_mo(0, first_pass=32, need_mo=0)),
    ("mid0-T48", dict(DENSE, prefill_mid=0, T=48), rows_mo(0, first_pass=32, need_mo=0)),
    ("mid0-T49", dict(DENSE, prefill_mid=0, T=49), big()),
    ("mid0-chunk0-T47", dict(DENSE, prefill_mid=0, prefill_chunk=0, T=47), ops()),
    ("mid0-chunk0-T48", dict(DENSE, prefill_mid=0, prefill_chunk=0, T=48), big()),
    ("mid0-bigmin128-T128", dict(DENSE, prefill_mid=0, prefill_big_min=128, T=128), ops()),
    ("mid0-bigmin128-T129", dict(DENSE, prefill_mid=0, prefill_big_min=128, T=129), big()),
    ("mid0-bigmin8-T33", dict(DENSE, prefill_mid=0, prefill_big_min=8, T=33), big()),      # (never below 33 tokens)
    ("mid0-bigmin8-T20", dict(DENSE, prefill_mid=0, prefill_big_min=8, T=20), rows_mo(0)),
    # ---- prefill_mid_max / prefill_res_mid lowered
    ("midmax64-T64", dict(DENSE, prefill_mid_max=64, prefill_res_mid=96, T=64), mid()),
    ("midmax64-T65", dict(DENSE, prefill_mid_max=64, prefill_res_mid=96, T=65), big(need_mo=2, res=True)),
    ("midmax64-T96", dict(DENSE, prefill_mid_max=64, prefill_res_mid=96, T=96), big(need_mo=2, res=True)),
    ("midmax64-T97", dict(DENSE, prefill_mid_max=64, prefill_res_mid=96, T=97), big()),
    ("midmax40-T44", dict(DENSE, prefill_mid_max=40, T=44), rows_mo(0, first_pass=32, need_mo=0)),      # (the mid route declines: two passes)
    ("resmid0-T1000", dict(DENSE, prefill_res_mid=0, T=1000), big()),
    # ---- each other option off
    ("big0-T40", dict(DENSE, prefill_big=0, T=40), rows_mo(0, first_pass=32, need_mo=0)),       # (k_gemm_mid rides on the large-tile route's conditions, P2)
    ("big0-T100", dict(DENSE, prefill_big=0, T=100), ops()),
    ("chunk0-T40", dict(DENSE, prefill_chunk=0, T=40), mid()),
    ("gemm_rows0-T8", dict(DENSE, gemm_rows=0, T=8), ops()),
    ("gemm_rows0-T40", dict(DENSE, gemm_rows=0, prefill_mid=0, T=40), ops()),
    ("batch_fused0-T8", dict(DENSE, batch_fused=0, T=8), ops()),
    ("splitk0-T100", dict(DENSE, gemm_splitk=0, T=100), mid(no_waits=1)),                      # (P6: the mid route reads the large tiles' option)
    ("splitk0-T1000", dict(DENSE, gemm_splitk=0, T=1000), big(need_mo=2, res=True, no_waits=1, res_no_waits=0)),
    ("kparts0-T1000", dict(DENSE, rows_kparts=0, T=1000), big(need_mo=2, res=True, no_waits=0, res_no_waits=1)),
    ("kparts0-T20", dict(DENSE, rows_kparts=0, T=20), rows_mo(0, no_waits=1)),
    ("kparts0-T100", dict(DENSE, rows_kparts=0, T=100), mid()),
    # ---- exact order (P1), a partition (P5), perf_stat (P5; P3 is still asked and still builds: both passes then go op by op)
    ("exact-T40", dict(DENSE, exact_order=1, T=40), route(EXACT)),
    ("topo-T8", dict(DENSE, topo=1, T=8), ops()),
    ("topo-T40", dict(DENSE, topo=1, T=40), ops()),
    ("topo-T1000", dict(DENSE, topo=1, T=1000), ops()),
    ("pstat-T8", dict(DENSE, perf_stat=1, T=8), ops()),
    ("pstat-T40", dict(DENSE, perf_stat=1, T=40), ops(need_mo=1)),
    ("pstat-T40-mid0", dict(DENSE, perf_stat=1, prefill_mid=0, T=40), route(OPS, first_pass=32)),
    ("pstat-T100", dict(DENSE, perf_stat=1, T=100), ops()),
    # ---- mixture of experts: never the rows GEMM or k_gemm_mid for a prompt, never two passes; the large tiles fuse the attention half (P7)
    ("moe-T8", dict(MOE, T=8), ops()),
    ("moe-T40", dict(MOE, T=40), ops()),
    ("moe-T100", dict(MOE, T=100), big()),
    ("moe-T1000", dict(MOE, T=1000), big()),
    # ---- the model facts false one at a time
    ("rows_layers0-T8", dict(DENSE, rows_layers=0, T=8), ops()),
    ("rows_layers0-T40-mid0", dict(DENSE, rows_layers=0, prefill_mid=0, T=40), ops()),
    ("rows_layers0-T100", dict(DENSE, rows_layers=0, T=100), mid()),
    ("b64-T8", dict(B64, T=8), rows_mo(1)),
    ("b64-T8-mo0", dict(B64, rows_mo=0, T=8), ops()),
    ("big_layers0-T8", dict(DENSE, big_layers=0, T=8), rows_mo(1)),
    ("big_layers0-T40", dict(DENSE, big_layers=0, T=40), rows_mo(0, first_pass=32, need_mo=0)),
    ("big_layers0-T100", dict(DENSE, big_layers=0, T=100), ops()),
    # the copies are built before the shapes are looked at (P2): need_mo 1 on whatever route follows
    ("mid_shapes0-T33", dict(DENSE, mid_shapes=0, T=33), ops(need_mo=1)),
    ("mid_shapes0-T40", dict(DENSE, mid_shapes=0, T=40), rows_mo(0, first_pass=32, need_mo=1)),
    ("mid_shapes0-T100", dict(DENSE, mid_shapes=0, T=100), big(need_mo=1)),
    ("mid_shapes0-T1000", dict(DENSE, mid_shapes=0, T=1000), big(need_mo=2)),
]


@pytest.mark.parametrize("name,facts,want", TABLE, ids=[t[0] for t in TABLE])
def test_prompt_route_table(name, facts, want):
    assert plan(facts) == want


def bfused(norm_fused, src=MO, chunk=0, captured=1, no_waits=0):
    return dict(kind=B_FUSED, chunk=chunk, norm_fused=norm_fused, captured=captured, gm_kernel=K_ROWS, gm_src=src, gm_mo=1 if src == MO else 0,
                gm_no_waits=no_waits, need_mo=1)


def bops(captured=0, chunk=0):
    return dict(kind=B_OPS, chunk=chunk, norm_fused=0, captured=captured, gm_kernel=0, gm_src=0, gm_mo=0, gm_no_waits=0, need_mo=0)


B_TABLE = [
    # ---- with MO copies: one fused step up to 32 rows, balanced chunks above (B3: 33 -> 17 + 16, 40 -> 20 + 20)
    ("n1", dict(B_DENSE, n=1), bops()),
    ("n2", dict(B_DENSE, n=2), bfused(1)),
    ("n16", dict(B_DENSE, n=16), bfused(1)),
    ("n17", dict(B_DENSE, n=17), bfused(0)),
    ("n32", dict(B_DENSE, n=32), bfused(0)),
    ("n33", dict(B_DENSE, n=33), bfused(0, chunk=17)),
    ("n40", dict(B_DENSE, n=40), bfused(0, chunk=20)),
    # ---- without: 16 rows per step (17 -> 9 + 8, 32 -> 16 + 16, 33 -> 11 + 11 + 11, 40 -> 14 + 14 + 12), the norm prologue to 8 rows
    ("mo0-n1", dict(B_DENSE, rows_mo=0, n=1), bops()),
    ("mo0-n2", dict(B_DENSE, rows_mo=0, n=2), bfused(1, src=TILED)),
    ("mo0-n16", dict(B_DENSE, rows_mo=0, n=16), bfused(0, src=TILED)),
    ("mo0-n17", dict(B_DENSE, rows_mo=0, n=17), bfused(0, src=TILED, chunk=9)),
    ("mo0-n32", dict(B_DENSE, rows_mo=0, n=32), bfused(0, src=TILED, chunk=16)),
    ("mo0-n33", dict(B_DENSE, rows_mo=0, n=33), bfused(0, src=TILED, chunk=11)),
    ("mo0-n40", dict(B_DENSE, rows_mo=0, n=40), bfused(0, src=TILED, chunk=14)),
    # a single step (forward_batch: a chunk, a draft step) never splits: 20 rows after a downgrade go op by op
    ("step-n20-mo0", dict(B_DENSE, may_chunk=0, rows_mo=0, n=20), bops()),
    ("step-n20", dict(B_DENSE, may_chunk=0, n=20), bfused(0)),
    # ---- captured or not (B5)
    ("graph0", dict(B_DENSE, graph=0, n=4), bfused(1, captured=0)),
    ("logits_out", dict(B_DENSE, logits_out=1, n=4), bfused(1, captured=0)),
    ("moe-fused", dict(B_DENSE, has_moe=1, n=4), bfused(1)),
    ("ops-batch_graph", dict(B_DENSE, batch_fused=0, batch_graph=1, n=4), bops(captured=1)),
    ("ops-batch_graph-moe", dict(B_DENSE, batch_fused=0, batch_graph=1, has_moe=1, n=4), bops()),
    ("ops-no-batch_graph", dict(B_DENSE, batch_fused=0, n=4), bops()),
    ("ops-n40", dict(B_DENSE, batch_fused=0, n=40), bops()),
    ("topo", dict(B_DENSE, topo=1, batch_graph=1, n=4), bops()),
    ("rows_layers0", dict(B_DENSE, rows_layers=0, n=4), bops()),
    ("b64", dict(B_DENSE, rows_layers=1, n=4), bfused(1)),
    ("b64-mo0", dict(B_DENSE, rows_layers=1, rows_mo=0, n=4), bops()),
    ("kparts0", dict(B_DENSE, rows_kparts=0, n=20), bfused(0, no_waits=1)),
    ("exact", dict(B_DENSE, exact_order=1, n=4), dict(bops(), kind=B_EXACT)),
]


@pytest.mark.parametrize("name,facts,want", B_TABLE, ids=[t[0] for t in B_TABLE])
def test_batch_route_table(name, facts, want):
    assert bplan(facts) == want


def test_bad_arguments_are_refused():
    import inferflow_amd as ia
    L = ia.lib()
    for fn, names, outs, base in ((L.ifa_prompt_route_plan, FACTS, OUT, DENSE), (L.ifa_batch_route_plan, B_FACTS, B_OUT, B_DENSE)):
        facts = (C.c_int * len(names))(*[int(base[k]) for k in names])
        out = (C.c_int * len(outs))()
        assert fn(facts, len(names) - 1, out, len(outs)) != 0
        assert fn(facts, len(names), out, len(outs) - 1) != 0
        assert fn(None, len(names), out, len(outs)) != 0
        assert fn(facts, len(names), out, len(outs)) == 0


def test_symbols_exported_and_bound():
    import inferflow_amd as ia
    for name in ("ifa_prompt_route_plan", "ifa_batch_route_plan", "ifa_model_prompt_route"):
        assert hasattr(ia.lib(), name), "missing symbol " + name
        assert name in _capi.SIGNATURES
