"""CPU-only checks of the prompt GEMM launch plans (csrc/ifa_gemm_plan.h) through the host-only entry points ifa_gemm_mid_plan /
ifa_gemm_big_plan: hand-written tables of what k_gemm_mid and k_gemm_big launch for the Llama-2-7B products on 256 CUs (the part counts
and tile shapes the launchers' comments state, the rest worked out by hand from the rules next to them), the workgroup cap at its edges,
the gated pair's doubled cap, the least steps of a part, the measurement settings, and every refusal."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import inferflow_amd as ia
from inferflow_amd import dtypes as dt
from tests import prompt_gemm_util as U

QKV, WO, W13, W2 = (4096, 4096, 4096), (4096,), (11008,), (4096,)
LDS4, LDS8 = 3 * (16384 + 4096 + 1024), 3 * (32768 + 4096 + 1024)


def parts(p):
    return [t[0] for t in p["tries"]]


# (name, T, rows, cols, epi) -> token tiles, weight tiles, parts of K in the order they are tried
MID_TABLE = [
    # wq | wk | wv: 96 weight tiles; one token tile: 192 workgroups of two parts (384 of four are more than one per CU)
    ("qkv", 33, QKV, 4096, U.PLAIN, 1, 96, [2, 1]),
    ("qkv", 128, QKV, 4096, U.PLAIN, 1, 96, [2, 1]),
    ("qkv", 129, QKV, 4096, U.PLAIN, 2, 96, [1]),                   # 192 tiles: one part beats two
    ("qkv", 256, QKV, 4096, U.PLAIN, 2, 96, [1]),
    ("qkv", 512, QKV, 4096, U.PLAIN, 4, 96, [1]),
    ("qkv", 768, QKV, 4096, U.PLAIN, 6, 96, [1]),
    ("qkv", 1024, QKV, 4096, U.PLAIN, 8, 96, [1]),
    # wo: 32 weight tiles; one token tile: eight parts, 256 workgroups
    ("wo", 33, WO, 4096, U.RESIDUAL, 1, 32, [8, 4, 2, 1]),
    ("wo", 128, WO, 4096, U.RESIDUAL, 1, 32, [8, 4, 2, 1]),
    ("wo", 129, WO, 4096, U.RESIDUAL, 2, 32, [4, 2, 1]),
    ("wo", 256, WO, 4096, U.RESIDUAL, 2, 32, [4, 2, 1]),
    ("wo", 512, WO, 4096, U.RESIDUAL, 4, 32, [2, 1]),
    ("wo", 768, WO, 4096, U.RESIDUAL, 6, 32, [1]),
    ("wo", 1024, WO, 4096, U.RESIDUAL, 8, 32, [1]),
    # w2: the same tiles over 172 steps
    ("w2", 33, W2, 11008, U.RESIDUAL, 1, 32, [8, 4, 2, 1]),
    ("w2", 128, W2, 11008, U.RESIDUAL, 1, 32, [8, 4, 2, 1]),
    ("w2", 129, W2, 11008, U.RESIDUAL, 2, 32, [4, 2, 1]),
    ("w2", 512, W2, 11008, U.RESIDUAL, 4, 32, [2, 1]),
    ("w2", 768, W2, 11008, U.RESIDUAL, 6, 32, [1]),
    ("w2", 1024, W2, 11008, U.RESIDUAL, 8, 32, [1]),
    # w1 | w3: 172 tiles of 64 row pairs, two workgroups per CU: 344 workgroups of two parts
    ("w13", 33, W13, 4096, U.GLU, 1, 172, [2, 1]),
    ("w13", 128, W13, 4096, U.GLU, 1, 172, [2, 1]),
    ("w13", 129, W13, 4096, U.GLU, 2, 172, [1]),
    ("w13", 256, W13, 4096, U.GLU, 2, 172, [1]),
    ("w13", 512, W13, 4096, U.GLU, 4, 172, [1]),
    ("w13", 768, W13, 4096, U.GLU, 6, 172, [1]),
    ("w13", 1024, W13, 4096, U.GLU, 8, 172, [1]),
]


@pytest.mark.parametrize("name,T,rows,cols,epi,tm,tn,want", MID_TABLE, ids=["%s-%d" % (r[0], r[1]) for r in MID_TABLE])
def test_mid_llama2_7b(name, T, rows, cols, epi, tm, tn, want):
    p = U.mid_plan(T, rows, cols, epi, 256)
    assert p["error"] == 0 and p["ta"] == 4
    assert (p["tiles_m"], p["tiles_n"], p["ksteps"]) == (tm, tn, cols // 64)
    assert parts(p) == want
    assert [t[1] for t in p["tries"]] == [tm * tn * k for k in want]
    assert all(t[2] == LDS4 for t in p["tries"])
    if len(rows) == 3:
        assert p["tile0"] == [0, 32, 64, 96]
    else:
        assert p["tile0"] == [0, 1 << 30, 1 << 30, tn]          # (absent sets are never selected)


def test_mid_cap_edges():
    # 32 tiles x 8 parts == 256 == the cap of 256 CUs; of 255 CUs it is the cap + 1
    assert parts(U.mid_plan(128, (4096,), 2048, U.PLAIN, 256)) == [8, 4, 2, 1]
    assert parts(U.mid_plan(128, (4096,), 2048, U.PLAIN, 255)) == [4, 2, 1]
    # one tile more than the cap allows at 8 parts; at 4 parts 33 x 4 = 132 fits
    assert parts(U.mid_plan(128, (4096 + 16,), 2048, U.PLAIN, 256)) == [4, 2, 1]
    # 64 x 4 == 256, 65 x 4 == 260
    assert parts(U.mid_plan(128, (8192,), 2048, U.PLAIN, 256)) == [4, 2, 1]
    assert parts(U.mid_plan(128, (8192 + 16,), 2048, U.PLAIN, 256)) == [2, 1]
    # two token tiles count twice
    assert parts(U.mid_plan(129, (4096,), 2048, U.PLAIN, 256)) == [4, 2, 1]
    # the measurement setting two_per_cu doubles the cap of every epilogue
    assert parts(U.mid_plan(128, (8192,), 2048, U.PLAIN, 256, two_per_cu=1)) == [8, 4, 2, 1]
    n4, n8 = U.cap_edge_rows(2048, 33, 256)
    assert (n4, n8) == (4096 + 128, 4096)


def test_mid_gated_pair_has_twice_the_cap():
    # 64 tiles of 64 row pairs x 8 parts == 512 == 2 x 256
    assert parts(U.mid_plan(128, (4096,), 2048, U.GLU, 256)) == [8, 4, 2, 1]
    assert parts(U.mid_plan(128, (4096,), 2048, U.GLU, 255)) == [4, 2, 1]
    assert parts(U.mid_plan(128, (4096 + 64,), 2048, U.GLU, 256)) == [4, 2, 1]
    assert U.mid_plan(128, (4096,), 2048, U.GLU, 256)["tiles_n"] == 64
    # the plain epilogue on as many tiles (8192 rows): four parts
    assert parts(U.mid_plan(128, (8192,), 2048, U.PLAIN, 256)) == [4, 2, 1]
    assert parts(U.mid_plan(128, (4096,), 2048, U.GLU, 256, no_glu_split=1)) == [1]


@pytest.mark.parametrize("cols,want", [(256, [1]), (480 + 32, [2, 1]), (640, [2, 1]), (768, [2, 1]), (896, [2, 1]), (1024, [4, 2, 1]), (1152, [4, 2, 1]),
                                       (1920, [4, 2, 1]), (2048, [8, 4, 2, 1]), (2176, [8, 4, 2, 1]), (4096, [8, 4, 2, 1]), (4224, [8, 4, 2, 1])])
def test_mid_least_steps_of_a_part(cols, want):
    """ksteps / parts just below and at the minimum of 4: 30 steps give 3 per part at 8 parts, 32 give 4"""
    assert parts(U.mid_plan(33, (144,), cols, U.PLAIN, 256)) == want


def test_mid_settings():
    assert parts(U.mid_plan(33, (144,), 2048, U.PLAIN, 256, min_steps=8)) == [4, 2, 1]
    assert parts(U.mid_plan(33, (144,), 2048, U.PLAIN, 256, max_parts=2)) == [2, 1]
    assert parts(U.mid_plan(33, (144,), 4096, U.PLAIN, 256, max_parts=16)) == [16, 8, 4, 2, 1]
    assert parts(U.mid_plan(33, (144,), 4096 - 128, U.PLAIN, 256, max_parts=16)) == [8, 4, 2, 1]      # 62 steps: 3 per part at 16
    p = U.mid_plan(257, (144,), 4096, U.PLAIN, 256, max_parts=16, ta=8)
    assert p["ta"] == 8 and p["tiles_m"] == 2 and parts(p) == [8, 4, 2, 1] and p["tries"][0][2] == LDS8      # (no sixteen parts on the wide tile)
    assert U.mid_plan(257, (144,), 4096, U.PLAIN, 256)["tiles_m"] == 3
    assert parts(U.mid_plan(33, (144,), 2048, U.PLAIN, 256, no_waits=1)) == [1]
    assert parts(U.mid_plan(33, (144,), 2048, U.PLAIN, 256, waits_on=0)) == [1]


@pytest.mark.parametrize("over,err", [(dict(mo=0), 1), (dict(T=0), 2), (dict(nsets=0), 2), (dict(nsets=4), 2), (dict(nblk=4), 2), (dict(nblk=10), 2),
                                      (dict(rows0=24), 3), (dict(nsets=2, rows1=8), 3), (dict(epi=2, nsets=2, rows1=16), 4),
                                      (dict(epi=2, has_w1=0), 4), (dict(ld_or=4), 5), (dict(ld_or=8), 0)])
def test_mid_refusals(over, err):
    over = dict(over)
    p = U.mid_plan(over.pop("T", 33), (144,), 1024, over.pop("epi", U.PLAIN), 256, **over)
    assert p["error"] == err
    if err:
        assert p["tries"] == [] and p["tiles_n"] == 0


def shapes(p):
    return [(l["bm"], l["bn"], l["waves"], l["tn0"], l["tn_count"]) for l in p["launches"]]


# (name, T, rows, cols, epi) -> pick, launches (bm, bn, waves, tn0, tn_count), parts of K in order
BIG_TABLE = [
    # one token tile: 128 x 128 tiles, four parts of K where the tiles fill less than half the chip and K >= 4096; eight waves
    ("qkv", 33, QKV, 4096, U.PLAIN, 3, [(128, 128, 8, 0, 96)], [4, 1]),
    ("qkv", 128, QKV, 4096, U.PLAIN, 3, [(128, 128, 8, 0, 96)], [4, 1]),
    ("wo", 128, WO, 4096, U.RESIDUAL, 3, [(128, 128, 8, 0, 32)], [4, 1]),
    ("w2", 128, W2, 11008, U.RESIDUAL, 3, [(128, 128, 8, 0, 32)], [4, 1]),
    ("w13", 128, W13, 4096, U.GLU, 3, [(128, 128, 8, 0, 172)], [1]),
    # two token tiles: 192 tiles of wq | wk | wv are at least half the chip: two parts
    ("qkv", 129, QKV, 4096, U.PLAIN, 3, [(128, 128, 8, 0, 96)], [2, 1]),
    ("qkv", 256, QKV, 4096, U.PLAIN, 3, [(128, 128, 8, 0, 96)], [2, 1]),
    ("wo", 256, WO, 4096, U.RESIDUAL, 3, [(128, 128, 8, 0, 32)], [4, 1]),        # 64 tiles x 4 = one workgroup per CU
    ("w13", 256, W13, 4096, U.GLU, 2, [(128, 256, 8, 0, 86)], [1]),
    ("qkv", 512, QKV, 4096, U.PLAIN, 2, [(128, 256, 8, 0, 48)], [1]),
    ("wo", 512, WO, 4096, U.RESIDUAL, 3, [(128, 128, 8, 0, 32)], [2, 1]),         # 128 tiles, the last length with eight waves
    ("w13", 512, W13, 4096, U.GLU, 1, [(256, 256, 8, 0, 86)], [1]),
    ("wo", 768, WO, 4096, U.RESIDUAL, 3, [(128, 128, 4, 0, 32)], [2, 1]),
    ("w13", 768, W13, 4096, U.GLU, 1, [(256, 256, 8, 0, 85), (128, 256, 8, 85, 1)], [1]),
    ("qkv", 1024, QKV, 4096, U.PLAIN, 1, [(256, 256, 8, 0, 48)], [1]),
    ("wo", 1024, WO, 4096, U.RESIDUAL, 3, [(128, 128, 4, 0, 32)], [2, 1]),        # wo / w2 in two halves of K
    ("w2", 1024, W2, 11008, U.RESIDUAL, 3, [(128, 128, 4, 0, 32)], [2, 1]),
    ("w13", 1024, W13, 4096, U.GLU, 1, [(256, 256, 8, 0, 64), (128, 256, 8, 64, 22)], [1]),      # 86 weight tiles = 64 x 4 workgroups + 22 x 8
]


@pytest.mark.parametrize("name,T,rows,cols,epi,pick,want,ks", BIG_TABLE, ids=["%s-%d" % (r[0], r[1]) for r in BIG_TABLE])
def test_big_llama2_7b(name, T, rows, cols, epi, pick, want, ks):
    p = U.big_plan(T, rows, cols, dt.Q4_B32T1A, epi, 1, 256)
    assert p["error"] == 0 and p["stream_k"] == 0
    assert p["pick"] == pick and shapes(p) == want and p["ks"] == ks
    if len(want) == 2:
        assert (p["full_n"], p["rem_n"]) == (want[0][4], want[1][4])
    for l in p["launches"]:
        assert l["tiles_m"] == -(-T // l["bm"])
        assert l["lds"] == max(2 * (l["bm"] + l["bn"]) * 128, l["bm"] * (l["bn"] * 2 + 64))


def test_big_forced_shapes_and_switches():
    for force, want in ((1, (256, 256, 8)), (2, (128, 256, 8)), (3, (128, 128, 4)), (4, (64, 64, 4)), (5, (128, 64, 4)), (6, (64, 128, 4))):
        p = U.big_plan(150, (136,), 2112, dt.Q4_B32T1A, U.RESIDUAL, 1 | (force << 8), 256)
        assert p["pick"] == force and shapes(p)[0][:3] == want and p["ks"] == [1] and len(p["launches"]) == 1
        assert shapes(p)[0][4] == -(-136 // want[1])
    # a forced shape never splits K, takes four waves, and has no second launch
    assert U.big_plan(128, WO, 4096, dt.Q4_B32T1A, U.RESIDUAL, 1 | (3 << 8), 256)["ks"] == [1]
    assert len(U.big_plan(1024, W13, 4096, dt.Q4_B32T1A, U.GLU, 1 | (1 << 8), 256)["launches"]) == 1
    # 64-value blocks: no 256 x 256 and no small tiles (they would spill): forced 1 runs 128 x 256, forced 4 - 6 run 128 x 128
    assert shapes(U.big_plan(300, (512,), 2048, dt.Q6_B64T1, U.PLAIN, 1 | (1 << 8), 256))[0][:2] == (128, 256)
    assert shapes(U.big_plan(300, (512,), 2048, dt.Q6_B64T1, U.PLAIN, 1 | (4 << 8), 256))[0][:3] == (128, 128, 4)
    # bit 12, no_waits and waits off: no parts of K
    for kw in (dict(tiles_bits=1 | (1 << 12)), dict(no_waits=1), dict(waits_on=0)):
        assert U.big_plan(128, WO, 4096, dt.Q4_B32T1A, U.RESIDUAL, num_cus=256, **kw)["ks"] == [1]
    # the shapes the edge case list names: two token tiles x 64 weight tiles at K 2048; 48 and 128 tokens x 128 rows at K 4096; 513 tokens
    assert U.big_plan(256, (8192,), 2048, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)["ks"] == [2, 1]
    assert U.big_plan(256, (8192,), 1984, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)["ks"] == [1]            # K below 2048
    assert U.big_plan(256, (8192 - 128,), 2048, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)["ks"] == [1]       # 126 tiles: under half the chip
    assert U.big_plan(48, (128,), 4096, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)["ks"] == [4, 1]
    assert U.big_plan(128, (128,), 4032, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)["ks"] == [1]
    assert shapes(U.big_plan(512, (128,), 256, dt.Q4_B32T1A, U.RESIDUAL, 1, 256))[0][:3] == (128, 128, 8)
    assert shapes(U.big_plan(513, (128,), 256, dt.Q4_B32T1A, U.RESIDUAL, 1, 256))[0][:3] == (128, 128, 4)
    # the two-launch form first occurs, at <= 256 tokens and 256 CUs, at 257 weight tiles of 256 rows: one round of 256 + 1
    n2 = U.two_launch_rows(256, 256, 256)
    assert n2 == 257 * 256
    p = U.big_plan(256, (n2,), 256, dt.Q4_B32T1A, U.RESIDUAL, 1, 256)
    assert shapes(p) == [(256, 256, 8, 0, 256), (128, 256, 8, 256, 1)]
    # stream-K stays opt-in: bit 13 on a shape it was built for
    assert U.big_plan(1024, W13, 4096, dt.Q4_B32T1A, U.GLU, 1, 256)["stream_k"] == 0
    assert U.big_plan(1024, W13, 4096, dt.Q4_B32T1A, U.GLU, 1 | (1 << 13), 256)["stream_k"] == 1


@pytest.mark.parametrize("kw,err", [(dict(dtype=dt.F32), 1), (dict(nblk=3, dtype=dt.Q4_B32T1A), 1), (dict(T=0), 2), (dict(nsets=4), 2),
                                    (dict(dtype=dt.Q8_B32T2, epi=1), 3), (dict(epi=2, nsets=2, rows1=16), 4), (dict(epi=2, has_w1=0), 4),
                                    (dict(rows0=12), 5), (dict(ld_or=4), 6), (dict(dtype=dt.F16), 0), (dict(dtype=dt.Q4_B16), 0)])
def test_big_refusals(kw, err):
    kw = dict(kw)
    p = U.big_plan(kw.pop("T", 150), (136,), 192, kw.pop("dtype", dt.Q4_B32T1A), kw.pop("epi", U.PLAIN), 1, 256, **kw)
    assert p["error"] == err
    if err:
        assert p["launches"] == [] and p["ks"] == []


def test_entries_check_their_arguments():
    L = ia.lib()
    for fn, nf, no in ((L.ifa_gemm_mid_plan, 18, 25), (L.ifa_gemm_big_plan, 14, 23)):
        facts, out = (C.c_int * nf)(), (C.c_int * no)()
        assert fn(facts, nf - 1, out, no) != 0
        assert fn(facts, nf, out, no - 1) != 0
        assert fn(None, nf, out, no) != 0
        assert fn(facts, nf, out, no) != 0          # no CUs
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "inferflow_amd.h")).read()
    for name in ("ifa_gemm_mid_plan", "ifa_gemm_big_plan"):
        assert name in hdr


def test_plan_header_is_plain_cxx(tmp_path):
    """csrc/ifa_gemm_plan.h compiles with a plain host compiler: no HIP header, no HIP call"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "plan.cc"
    src.write_text('#include "ifa_gemm_plan.h"\nint main() { ifa::GemmMidFacts f; f.T = 33; f.rows0 = 144; f.nblk = 64; f.num_cus = 256;\n'
                   '  ifa::GemmBigFacts g; g.T = 150; g.rows0 = 136; g.nblk = 6; g.num_cus = 256;\n'
                   '  return !(ifa::plan_gemm_mid(f).parts[0] == 8 && ifa::plan_gemm_big(g).error == 0); }\n')
    inc = os.path.join(os.path.dirname(__file__), "..", "inferflow_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "plan")])
    subprocess.check_call([str(tmp_path / "plan")])
