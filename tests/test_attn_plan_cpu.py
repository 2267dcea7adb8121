"""CPU-only checks of the prompt attention launch plan (csrc/ifa_attn_plan.h) through the host-only entry point ifa_attention_plan:
hand-written tables of which kernel ifa_attention runs for the Llama-2-7B heads (32 x 128) and a 64-wide geometry at 1 .. 128 queries
and the key counts around every limit, with grid, LDS bytes and workspace; the last context of the LDS score tile per head size, from the
formula and by search over the plan; both settings; the rows entry; every refusal."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import inferflow_amd as ia
from inferflow_amd import dtypes as dt
from tests import prompt_attn_util as U

F16, Q8 = dt.F16, dt.Q8_B32T2
SC, LDS, WS, TP64, TP128 = U.SCALAR, U.MFMA_LDS, U.MFMA_WS, U.TWO_PASS64, U.TWO_PASS128
L7B, G64 = (32, 32, 128), (8, 2, 64)
LDS2P_128 = 4 * 32 * 128 * 2 + 4 * 128 * 40 * 2          # [2 stages][2 parities] K blocks of 32 x 128 halfs, then V blocks of 128 x 40: 73728
LDS2P_64 = 4 * 32 * 64 * 2 + 4 * 64 * 40 * 2              # 36864


def scalar_lds(n):
    return (n * 2 + 15) // 16 * 16 + 64


def tile_lds(n, hd):
    return 32 * ((n + 31) // 32 * 32 + 8) * 2 + hd * 40 * 2 + 64


def P(geo, q, n, settings=U.DEFAULT_SETTINGS, kvd=F16, prefix=None):
    return U.plan(kvd, n, q, n - q if prefix is None else prefix, *geo, settings=settings)


# (geometry, queries, keys) -> kind, queries per workgroup, grid x, LDS bytes; grid y = heads but for the scalar kernel (heads, queries)
TABLE = [
    # fewer than 4 queries: the scalar kernel at every length
    (L7B, 1, 1, SC, 1, 32, scalar_lds(1)), (L7B, 1, 4096, SC, 1, 32, scalar_lds(4096)), (L7B, 3, 2209, SC, 1, 32, scalar_lds(2209)),
    (G64, 1, 7, SC, 1, 8, 80), (G64, 3, 3, SC, 1, 8, 80), (G64, 3, 65536, SC, 1, 8, 131072 + 64),
    # 4 .. 63 queries: 32-query tiles, the score tile in the LDS up to 2208 keys (128-wide) / 2304 keys (64-wide), then the workspace
    (L7B, 4, 4, LDS, 32, 1, tile_lds(4, 128)), (L7B, 4, 2208, LDS, 32, 1, 152128), (L7B, 4, 2209, WS, 32, 1, 10304),
    (L7B, 63, 63, LDS, 32, 2, tile_lds(63, 128)), (L7B, 63, 2208, LDS, 32, 2, 152128), (L7B, 63, 2209, WS, 32, 2, 10304), (L7B, 63, 4096, WS, 32, 2, 10304),
    (G64, 4, 2304, LDS, 32, 1, 153152), (G64, 4, 2305, WS, 32, 1, 5184), (G64, 63, 2304, LDS, 32, 2, 153152), (G64, 63, 2305, WS, 32, 2, 5184),
    (G64, 33, 33, LDS, 32, 2, tile_lds(33, 64)),
    # from 64 queries: the two-pass kernel with 64 queries per workgroup, at every length (nothing of size n_keys is stored)
    (L7B, 64, 64, TP64, 64, 1, LDS2P_128), (L7B, 64, 2209, TP64, 64, 1, LDS2P_128), (L7B, 127, 127, TP64, 64, 2, LDS2P_128),
    (L7B, 128, 128, TP64, 64, 2, LDS2P_128), (L7B, 128, 4096, TP64, 64, 2, LDS2P_128), (L7B, 129, 65536, TP64, 64, 3, LDS2P_128),
    (G64, 64, 64, TP64, 64, 1, LDS2P_64), (G64, 127, 2305, TP64, 64, 2, LDS2P_64), (G64, 128, 128, TP64, 64, 2, LDS2P_64),
]


@pytest.mark.parametrize("geo,q,n,kind,qpw,gx,lds", TABLE, ids=["h%d-hd%d-q%d-n%d" % (r[0][0], r[0][2], r[1], r[2]) for r in TABLE])
@pytest.mark.parametrize("kvd", [F16, Q8], ids=["f16", "q8"])
def test_kinds_by_default(geo, q, n, kind, qpw, gx, lds, kvd):
    p = P(geo, q, n, kvd=kvd)
    assert p["error"] == 0 and (p["kind"], p["q_per_wg"], p["lds"]) == (kind, qpw, lds), p
    assert p["grid"] == ((geo[0], q) if kind == SC else (gx, geo[0]))
    assert p["xcd_remap"] == (0 if kind == SC else 1)         # (32 and 8 heads: an XCD keeps an eighth of them)
    if kind == WS:
        nkp = (n + 31) // 32 * 32 + 8
        assert p["sg_nkp"] == nkp and p["ws_bytes"] == geo[0] * gx * 32 * nkp * 2
    else:
        assert p["sg_nkp"] == 0 and p["ws_bytes"] == 0
    # the cache rows behind the queries do not matter, only their count: any prefix gives the same launch
    assert P(geo, q, n, kvd=kvd, prefix=0) == p


@pytest.mark.parametrize("hd,want", [(32, 2336), (64, 2304), (128, 2208)])
def test_last_context_of_the_lds_tile(hd, want):
    """150 KiB - 64 - the V block leave 32 rows of pf_nkp halfs: the key count grows by whole 32-blocks (+ 8 halfs of padding)"""
    assert U.last_lds_ctx(hd) == want
    assert U.mfma_lds_bytes(want, hd) <= 150 * 1024 < U.mfma_lds_bytes(want + 1, hd)
    geo = (8, 8, hd)
    kinds = [P(geo, 40, n)["kind"] for n in range(40, 4200)]           # (40 queries: under the two-pass threshold)
    found = max(n for n, k in zip(range(40, 4200), kinds) if k == LDS)
    assert found == want
    assert all(k == (LDS if n <= want else WS) for n, k in zip(range(40, 4200), kinds))         # one switch, no island
    assert P(geo, 40, want)["lds"] == U.mfma_lds_bytes(want, hd) and P(geo, 40, want + 1)["lds"] == hd * 80 + 64
    assert P(geo, 4, 65536)["kind"] == WS


def test_head_sizes():
    # 32-wide heads have no two-pass kernel: the staged one at every query count
    assert P((8, 8, 32), 64, 64)["kind"] == LDS and P((8, 8, 32), 300, 2337)["kind"] == WS and P((8, 8, 32), 300, 2336)["kind"] == LDS
    assert P((8, 8, 32), 300, 2337)["grid"] == (10, 8)
    # other head sizes: the scalar kernel whatever the chunk
    for hd in (16, 48, 80, 96, 256):
        for q, n in ((1, 1), (5, 5), (70, 300), (200, 3000)):
            p = P((4, 2, hd), q, n)
            assert (p["kind"], p["grid"], p["lds"], p["xcd_remap"]) == (SC, (4, q), scalar_lds(n), 0)
    # 6 and 4 heads: the plain (tile, head) mapping
    assert P((6, 3, 64), 64, 64)["xcd_remap"] == 0 and P((4, 1, 128), 40, 40)["xcd_remap"] == 0 and P((16, 2, 64), 40, 40)["xcd_remap"] == 1


def test_settings():
    # ifa_attention_two_pass_min(0): never (stored as 1 << 30): the staged kernel at every chunk
    assert P(L7B, 64, 64, U.FORCE_STAGED)["kind"] == LDS and P(L7B, 4096, 4096, U.FORCE_STAGED)["kind"] == WS
    assert P(L7B, 4096, 4096, U.FORCE_STAGED)["grid"] == (128, 32)
    # a lower and a higher threshold
    assert P(G64, 32, 32, (32, U.NEVER))["kind"] == TP64 and P(G64, 31, 31, (32, U.NEVER))["kind"] == LDS
    assert P(G64, 32, 32, (32, U.NEVER))["grid"] == (1, 8)
    assert P(G64, 199, 199, (200, U.NEVER))["kind"] == LDS and P(G64, 200, 200, (200, U.NEVER))["kind"] == TP64
    assert P(G64, 3, 3, (1, U.NEVER))["kind"] == TP64           # (the threshold alone decides: no lower limit of its own)
    # ifa_attention_two_pass_min_keys: the 128-query variant from 128 queries and that many keys on
    p = P(L7B, 128, 128, U.FORCE_128)
    assert (p["kind"], p["q_per_wg"], p["grid"], p["lds"], p["xcd_remap"]) == (TP128, 128, (1, 32), 0, 1)
    assert P(L7B, 129, 500, U.FORCE_128)["grid"] == (2, 32) and P(L7B, 127, 500, U.FORCE_128)["kind"] == TP64
    assert P(L7B, 128, 1023, (64, 1024))["kind"] == TP64 and P(L7B, 128, 1024, (64, 1024))["kind"] == TP128
    assert P(L7B, 127, 4096, (64, 1024))["kind"] == TP64
    # the variant needs the two-pass threshold too
    assert P(L7B, 128, 128, (200, 0))["kind"] == LDS and P(L7B, 200, 200, (200, 0))["kind"] == TP128
    assert P((8, 8, 32), 128, 128, U.FORCE_128)["kind"] == LDS
    # the two setters hand back what the plan reads, and the library starts with the defaults
    L = ia.lib()
    assert (L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1)) == U.DEFAULT_SETTINGS
    prev = L.ifa_attention_two_pass_min(0)
    try:
        assert (L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1)) == U.FORCE_STAGED
    finally:
        L.ifa_attention_two_pass_min(prev)
    prev = L.ifa_attention_two_pass_min_keys(0)
    try:
        assert (L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1)) == U.FORCE_128
    finally:
        L.ifa_attention_two_pass_min_keys(prev)
    assert (L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1)) == U.DEFAULT_SETTINGS


def test_workspace_bytes_past_32_bits():
    p = P(L7B, 65535, 65536, U.FORCE_STAGED)
    assert p["kind"] == WS and p["grid"] == (2048, 32) and p["sg_nkp"] == 65544
    assert p["ws_bytes"] == 32 * 2048 * 32 * 65544 * 2 > 1 << 32


def test_rows_mode():
    """ifa_attention_rows: the scalar kernel, a workgroup per (head, row), the LDS sized by the longest context of the batch"""
    for rows, max_ctx in ((1, 1), (5, 600), (8, 257), (300, 4096)):
        p = U.plan(Q8, max_ctx, rows, 0, 8, 2, 64, rows_mode=1)
        assert (p["error"], p["kind"], p["q_per_wg"], p["grid"], p["lds"], p["xcd_remap"], p["ws_bytes"]) == (0, SC, 1, (8, rows), scalar_lds(max_ctx), 0, 0)
    assert U.plan(F16, 600, 0, 0, 8, 2, 64, rows_mode=1)["error"] == 4 and U.plan(F16, 0, 5, 0, 8, 2, 64, rows_mode=1)["error"] == 4


REFUSALS = [
    (dict(kvd=dt.F32), 1), (dict(kvd=dt.Q4_B32T1A), 1), (dict(kvd=dt.Q8_B32T1), 1),
    (dict(heads=0), 2), (dict(kv_heads=0), 2), (dict(kv_heads=3), 2), (dict(heads=-8), 2),
    (dict(hd=0), 3), (dict(kv_heads=1, hd=48), 3), (dict(kv_heads=1, hd=16), 3),
    (dict(n=0), 4), (dict(q=0), 4), (dict(prefix=-1), 4), (dict(n=-5), 4),
    (dict(n=65537), 5), (dict(q=65536, n=65536), 5),
    (dict(n=65536, q=65535), 0), (dict(kv_heads=2, hd=48), 0), (dict(kvd=Q8), 0), (dict(prefix=0), 0),
]


@pytest.mark.parametrize("over,err", REFUSALS, ids=["%s-%d" % ("-".join("%s%s" % kv for kv in r[0].items()), r[1]) for r in REFUSALS])
def test_refusals(over, err):
    a = dict(kvd=F16, n=300, q=70, prefix=230, heads=8, kv_heads=2, hd=64)
    a.update(over)
    p = U.plan(a["kvd"], a["n"], a["q"], a["prefix"], a["heads"], a["kv_heads"], a["hd"])
    assert p["error"] == err
    if err:
        assert (p["grid"], p["lds"], p["q_per_wg"], p["ws_bytes"]) == ((0, 0), 0, 0, 0)
        # ifa_attention refuses the same arguments with its error code, before it touches a device (nothing is launched)
        L = ia.lib()
        assert L.ifa_attention(1, 1, 1, a["kvd"], a["n"], a["q"], a["prefix"], a["heads"], a["kv_heads"], a["hd"], 1.0, 0, 0, 0, 1, None) == -1
        assert b"ifa_attention" in L.ifa_last_error()


def test_entries_check_their_arguments():
    L = ia.lib()
    facts, out = (C.c_int * 10)(F16, 300, 70, 230, 8, 2, 64, 64, 1 << 30, 0), (C.c_int * 10)()
    assert L.ifa_attention_plan(facts, 10, out, 10) == 0 and out[1] == TP64
    assert L.ifa_attention_plan(facts, 9, out, 10) != 0 and L.ifa_attention_plan(facts, 10, out, 9) != 0
    assert L.ifa_attention_plan(None, 10, out, 10) != 0 and L.ifa_attention_plan(facts, 10, None, 10) != 0
    assert L.ifa_attention(None, 1, 1, F16, 300, 70, 230, 8, 2, 64, 1.0, 0, 0, 0, 1, None) == -1
    assert L.ifa_attention(1, 1, 1, F16, 300, 70, 230, 8, 2, 64, 0.0, 0, 0, 0, 1, None) == -1 and b"kq_scale" in L.ifa_last_error()
    assert L.ifa_attention_rows(None, 1, F16, 5, 600, 8, 2, 64, 1.0, 0, 0, 0, 1, None) == -1
    assert L.ifa_attention_rows(1, 1, F16, 0, 600, 8, 2, 64, 1.0, 0, 0, 0, 1, None) == -1
    assert L.ifa_attention_rows(1, 1, F16, 5, 0, 8, 2, 64, 1.0, 0, 0, 0, 1, None) == -1
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "inferflow_amd.h")).read()
    assert "ifa_attention_plan" in hdr and "ifa_attention_rows" in hdr


def test_plan_header_is_plain_cxx(tmp_path):
    """csrc/ifa_attn_plan.h compiles with a plain host compiler: no HIP header, no HIP call"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "plan.cc"
    src.write_text('#include "ifa_attn_plan.h"\nint main() { ifa::AttnFacts f; f.n_ctx = 2209; f.q_tokens = 40; f.prefix_len = 2169; f.heads = 2; f.kv_heads = 1;\n'
                   '  f.head_dim = 128; const ifa::AttnPlan p = ifa::plan_attention(f); f.q_tokens = 64; const ifa::AttnPlan t = ifa::plan_attention(f);\n'
                   '  f.heads = 0; static_assert(ifa::ATTN_N_FACTS == 10 && ifa::ATTN_N_OUT == 10, "array sizes");\n'
                   '  return !(p.kind == ifa::ATTN_MFMA_WORKSPACE && p.sg_nkp == 2248 && p.ws_bytes == 575488 && p.lds == 10304 && t.kind == ifa::ATTN_TWO_PASS64\n'
                   '           && ifa::plan_attention(f).error == ifa::ATTN_ERR_HEADS && ifa::pf_nkp(33) == 72); }\n')
    inc = os.path.join(os.path.dirname(__file__), "..", "inferflow_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "plan")])
    subprocess.check_call([str(tmp_path / "plan")])
