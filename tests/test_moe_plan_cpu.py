"""CPU-only: the plan of a mixture-of-experts layer (csrc/ifa_moe_plan.h, rules M1 - M10 of DESIGN.md "MoE layer plan") through the
host-only entry point ifa_moe_plan, against values written by hand from the rules: the row counts at which a field flips for the
test_moe widths and for Mixtral-8x7B's, every option / table / predicate flipped alone, the router's conditions, invariants over a sweep,
the entries' argument checks, and the header as plain C++ (tests/moe_plan_sweep.cc: the same invariants over every setting)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import inferflow_amd as ia
from inferflow_amd import dtypes as dt
from inferflow_amd.worker import MOE_FACTS, MOE_PLAN_FIELDS, moe_plan

# a layer with everything in place: tiled Q4 experts, all three pointer tables, every option at its default, the fused batched step calling
COMMON = dict(w_dtype=dt.Q4_B32T1A, w_ax8=1, w_q4=1, full_quant_gemv=1, norm_kind=0, gate_f16=1, gate_cols_match=1, has_ffn_norm=1,
              experts_uniform=1, have_table=1, have_table_aos=1, have_table_mo=1, moe_device=1, moe_router_fused=1, moe_singles=1, moe_overlap=1,
              gemm_rows=1, rows_mo=1, rows_use_mfma=1, rows_mfma_ok=1, rows_q4_ok=1, singles_ok=1, caller_norm=1)
SMALL = dict(COMMON, experts=4, top_k=2, dim=256, ffn=512)             # synth "test_moe"
MIXTRAL = dict(COMMON, experts=8, top_k=2, dim=4096, ffn=14336)


def host(cap, router="ops", device_ok=1):
    return dict(kind="host", router=router, device_ok=device_ok, cap=cap, tile_rows=0, small_max=0, max_tiles=0, max_singles=0, max_smalls=0,
                rows_kernel=0, rows_mfma=0, smalls_mo=0, side_stream=0, host_sync=1)


def dev(kind, router, cap, tile_rows, small_max, max_tiles, max_singles, max_smalls, smalls_mo, side_stream, rows_mfma=1):
    return dict(kind="device_" + kind, router=router, device_ok=1, cap=cap, tile_rows=tile_rows, small_max=small_max, max_tiles=max_tiles,
                max_singles=max_singles, max_smalls=max_smalls, rows_kernel=1 if small_max else 0, rows_mfma=rows_mfma, smalls_mo=smalls_mo,
                side_stream=side_stream, host_sync=0)


#  (base, T) ->                     kind       router   cap  tile small tiles singles smalls mo side
ROWS = [
    (SMALL, 1, host(2, "fused")),                                              # one row: host-routed; the decode step's router is the one launch
    (SMALL, 2, dev("singles", "fused", 4, 64, 8, 0, 4, 2, 1, 1)),               # the device route starts; 4 pairs: at most 2 groups of 2 rows
    (SMALL, 8, dev("singles", "fused", 16, 64, 8, 0, 4, 4, 1, 1)),              # the last step no expert of which can collect more than 8 rows
    (SMALL, 9, dev("grouped", "fused", 18, 64, 8, 4, 4, 4, 1, 0)),              # tiles possible: 18 / 64 + 4 of them, and with them the grouped route
    (SMALL, 16, dev("grouped", "fused", 32, 64, 8, 4, 4, 4, 1, 0)),             # 32 pairs = 8 x 4 experts: the last step with small groups
    (SMALL, 17, dev("grouped", "fused", 34, 64, 0, 4, 4, 0, 0, 0)),
    (SMALL, 32, dev("grouped", "fused", 64, 64, 0, 5, 4, 0, 0, 0)),             # the last step of the rows router
    (SMALL, 33, dev("grouped", "ops", 66, 64, 0, 5, 4, 0, 0, 0)),
    (SMALL, 191, dev("grouped", "ops", 382, 64, 0, 9, 4, 0, 0, 0)),             # 95 rows per expert on average
    (SMALL, 192, dev("grouped", "ops", 384, 128, 0, 7, 4, 0, 0, 0)),            # 96: 128-row tiles
    (MIXTRAL, 1, host(2, "fused")),
    (MIXTRAL, 2, dev("singles", "fused", 4, 64, 8, 0, 4, 2, 1, 1)),
    (MIXTRAL, 8, dev("singles", "fused", 16, 64, 8, 0, 8, 8, 1, 1)),
    (MIXTRAL, 9, dev("grouped", "fused", 18, 64, 8, 8, 8, 8, 1, 0)),
    (MIXTRAL, 32, dev("grouped", "fused", 64, 64, 8, 9, 8, 8, 1, 0)),           # 64 pairs = 8 x 8 experts, and the router's 32 rows
    (MIXTRAL, 33, dev("grouped", "ops", 66, 64, 0, 9, 8, 0, 0, 0)),
    (MIXTRAL, 383, dev("grouped", "ops", 766, 64, 0, 19, 8, 0, 0, 0)),
    (MIXTRAL, 384, dev("grouped", "ops", 768, 128, 0, 14, 8, 0, 0, 0)),
]


@pytest.mark.parametrize("base,T,want", ROWS, ids=["%s-T%d" % ("small" if r[0] is SMALL else "mixtral", r[1]) for r in ROWS])
def test_rows_at_which_a_field_flips(base, T, want):
    assert moe_plan(T=T, **base) == want


M8 = dev("singles", "fused", 16, 64, 8, 0, 8, 8, 1, 1)                         # Mixtral, 8 rows, everything on (ROWS above)
# no small groups at all: every pair may need a tile (16 / 64 + 8), so the grouped route
NO_SMALLS = dev("grouped", "fused", 16, 64, 0, 8, 8, 0, 0, 0)
# small groups, but from the tiled layout (three launches + the element-wise gate): the singles cannot have the quantiser to themselves
TILED_SMALLS = dev("grouped", "fused", 16, 64, 8, 0, 8, 8, 0, 0)
FLIPS = [
    ("moe_device", 0, host(16, device_ok=0)),
    ("moe_router_fused", 0, dict(M8, router="ops")),
    ("moe_singles", 0, dict(M8, kind="device_grouped", side_stream=0)),
    ("moe_overlap", 0, dict(M8, side_stream=0)),
    ("gemm_rows", 0, NO_SMALLS),
    ("rows_mo", 0, TILED_SMALLS),
    ("have_table", 0, NO_SMALLS),
    ("have_table_aos", 0, host(16, device_ok=0)),
    ("have_table_mo", 0, TILED_SMALLS),
    ("rows_use_mfma", 0, dict(TILED_SMALLS, rows_mfma=0)),                      # the fdot2 rows kernel takes the small groups (rows_q4_ok)
    ("rows_mfma_ok", 0, dict(TILED_SMALLS, rows_mfma=0)),
    ("rows_q4_ok", 0, M8),                                                      # (only read where the matrix-core variant is out)
    ("singles_ok", 0, dict(M8, kind="device_grouped", side_stream=0)),
    ("experts_uniform", 0, host(16, device_ok=0)),
    ("w_ax8", 0, host(16, device_ok=0)),
    ("w_q4", 0, NO_SMALLS),
    ("full_quant_gemv", 0, host(16, device_ok=0)),
    ("caller_norm", 0, dict(M8, router="ops")),                                 # the op-by-op layer normalises the rows itself
    ("ffn", 14352, host(16, device_ok=0)),                                      # % 32 != 0
]


@pytest.mark.parametrize("name,value,want", FLIPS, ids=["%s-%d" % r[:2] for r in FLIPS])
def test_each_fact_flipped_alone(name, value, want):
    assert moe_plan(T=8, **MIXTRAL) == M8
    assert moe_plan(T=8, **dict(MIXTRAL, **{name: value})) == want


def test_neither_rows_kernel_means_no_small_groups():
    assert moe_plan(T=8, **dict(MIXTRAL, rows_use_mfma=0, rows_q4_ok=0)) == dict(NO_SMALLS, rows_mfma=0)
    assert moe_plan(T=8, **dict(MIXTRAL, rows_mfma_ok=0, rows_q4_ok=0)) == dict(NO_SMALLS, rows_mfma=0)


# what k_dec_moe_router covers (M3 - M5): (facts over MIXTRAL) -> router at one row, router at 8 rows of the fused batched step
ROUTER = [
    (dict(), "fused", "fused"),
    (dict(norm_kind=1), "ops", "ops"),
    (dict(gate_f16=0), "ops", "ops"),
    (dict(gate_cols_match=0), "ops", "ops"),
    (dict(has_ffn_norm=0), "fused", "ops"),                                     # one row: the kernel copies instead (eps < 0)
    (dict(caller_norm=0), "fused", "ops"),
    (dict(dim=16384 + 32), "ops", "ops"),
    (dict(dim=4096 + 8), "fused", "ops"),                                       # % 8 == 0 but not % 32: host-routed rows, whose router is the ops'
    (dict(dim=4096 + 4), "ops", "ops"),
    (dict(experts=64), "fused", "fused"),
    (dict(experts=65), "ops", "ops"),
    (dict(moe_device=0), "fused", "ops"),
]


@pytest.mark.parametrize("over,one,rows", ROUTER, ids=["-".join("%s%s" % kv for kv in r[0].items()) or "default" for r in ROUTER])
def test_router(over, one, rows):
    assert moe_plan(T=1, **dict(MIXTRAL, **over))["router"] == one
    assert moe_plan(T=8, **dict(MIXTRAL, **over))["router"] == rows


def test_invariants_over_a_sweep():
    L = ia.lib()
    names = list(MOE_FACTS)
    opts = [names.index(n) for n in ("moe_device", "moe_router_fused", "moe_singles", "moe_overlap", "gemm_rows", "rows_mo")]
    iT, iE, iK = names.index("T"), names.index("experts"), names.index("top_k")
    KIND, TILES, SMALLS, MFMA, MO, SIDE, SYNC = (MOE_PLAN_FIELDS.index(n) for n in
                                                 ("kind", "max_tiles", "max_smalls", "rows_mfma", "smalls_mo", "side_stream", "host_sync"))
    facts = (C.c_int * len(names))(*[int(dict(MIXTRAL, T=1)[n]) for n in names])
    out = (C.c_int * len(MOE_PLAN_FIELDS))()
    kinds = set()
    for E in (4, 8, 64):
        for K in (1, 2, 8):
            facts[iE], facts[iK] = E, K
            for bits in range(64):
                for b, i in enumerate(opts):
                    facts[i] = (bits >> b) & 1
                for T in range(1, 513):
                    facts[iT] = T
                    assert L.ifa_moe_plan(facts, len(names), out, len(out)) == 0
                    p = out[:]
                    ok = (p[SMALLS] <= E and (not p[MO] or p[MFMA]) and (not p[SIDE] or p[KIND] == 2) and p[SYNC] == (p[KIND] == 0)
                          and (p[KIND] != 2 or p[TILES] == 0))
                    assert ok, (E, K, bits, T, dict(zip(MOE_PLAN_FIELDS, p)))
                    kinds.add(p[KIND])
    assert kinds == {0, 1, 2}


def test_entries_check_their_arguments():
    L = ia.lib()
    nf, no = len(MOE_FACTS), len(MOE_PLAN_FIELDS)
    assert (nf, no) == (28, 14)
    facts, out = (C.c_int * nf)(*[int(dict(MIXTRAL, T=8)[n]) for n in MOE_FACTS]), (C.c_int * no)()
    assert L.ifa_moe_plan(facts, nf, out, no) == 0 and out[0] == 2 and out[3] == 16
    assert L.ifa_moe_plan(facts, nf - 1, out, no) != 0 and L.ifa_moe_plan(facts, nf + 1, out, no) != 0 and L.ifa_moe_plan(facts, nf, out, no - 1) != 0
    assert L.ifa_moe_plan(None, nf, out, no) != 0 and L.ifa_moe_plan(facts, nf, None, no) != 0
    assert b"ifa_moe_plan" in L.ifa_last_error()
    for name in ("T", "experts", "top_k"):
        bad = (C.c_int * nf)(*[int(dict(dict(MIXTRAL, T=8), **{name: 0})[n]) for n in MOE_FACTS])
        assert L.ifa_moe_plan(bad, nf, out, no) != 0, name
    assert L.ifa_model_moe_plan(None, 0, 2, 0, out, no) != 0 and b"ifa_model_moe_plan" in L.ifa_last_error()
    with pytest.raises(KeyError):
        moe_plan(T=8, **dict(MIXTRAL, no_such_fact=1))
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "inferflow_amd.h")).read()
    for name in ("ifa_moe_plan", "ifa_model_moe_plan"):
        assert hasattr(L, name) and "int %s(" % name in hdr, name


def test_plan_header_is_plain_cxx(tmp_path):
    """csrc/ifa_moe_plan.h compiles with a plain host compiler -- no HIP header, no HIP call, no engine state -- and the stand-alone sweep
    (every setting of the options, tables and predicates x rows 1..512) holds"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    here = os.path.dirname(__file__)
    inc = os.path.join(here, "..", "inferflow_amd", "csrc")
    exe = str(tmp_path / "moe_plan_sweep")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", inc, os.path.join(here, "moe_plan_sweep.cc"), "-o", exe])
    subprocess.check_call([exe])
