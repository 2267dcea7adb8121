"""CPU-only: the rows GEMM launch plan (csrc/ifa_gemm_rows_plan.h, through ifa_gemm_rows_plan) against tables written by hand from the
launchers, every refusal, and the proof that the assertions of tests/test_gpu_rows_gemm_edges.py cannot pass a faulty kernel: for every
launch shape of every case of the device test (tests/rows_gemm_util.model_cases at 256 CUs), every fault of RowsRef.faults moves the float64
value of at least one element by >= SENSITIVITY x the bound the device test applies, and the check rejects the oracle's output shifted by
that fault.  The seed check: with the RMS scale one fp32 ulp down or up, every norm-fused launch on scale-dependent inputs stays inside
F_FLIPS flips and the FLIP_ROWS_MAX cap.

Which instances a model reaches on 256 CUs (docs/rows_gemm_edges.md): dim <= 4096 keeps Wo and W2 at <= 256 tiles, one tile per workgroup,
so their K parts are the KPM 1 instances (2, 3, 4, 6, 8 tiles per group).  Only the QKV launch has more tiles than CUs, its K = dim <= 4096 is
one chunk up to 16 rows (no K parts) and two 2048-column chunks at 17..32 rows: two parts of two-tile workgroups, KPM 2 with 4 tiles per
group.  KPM 2 with 6 or 8 tiles needs 3 or 4 chunks on a launch of more tiles than CUs: no model on 256 CUs; the tables reach them at 64 and
32 CUs.  Every row count of a model is a multiple of 16 (QD % 128, KVD % 32 -- the engine asks KVD % 16 and heads of at least 32 --, dim % 128, ffn % 128): no partial tile through the engine."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, worker as Wk
from tests import rows_gemm_util as U

PLAIN, RES, GLU = U.PLAIN, U.RESIDUAL, U.GLU
TILED, MO = 0, 1
A = dt.Q4_B32T1A


def tries(p):
    return [tuple(t[k] for k in ("kparts", "kpm", "tiles", "groups", "grid", "lds", "scratch")) for t in p["tries"]]


def head(p):
    return tuple(p[k] for k in ("error", "ntiles", "tx", "ch", "chunk_cols", "nchunk"))


# (T, rows, K, epi, norm, layout, CUs, settings) -> (error, tiles, rows staged, CH, chunk columns, chunks), attempts in order:
# (kparts, KPM, tiles per workgroup or group, groups, grid, LDS bytes, scratch bytes).  LDS: MO tx rows x 8208 + 512 (32 rows: 32 x 4112);
# tiled tx rows x 8208 (16 rows: x 4112) + 8 patches of 5632 (16 rows: 3072) + 256; never less than tiles x 8192 (32 rows: x 16384).
TABLE = [
    # -- rows staged, one chunk (MO) against the chunk loop (tiled: always), the norm prologue
    ((2, (4096,), 4096, PLAIN, 0, MO, 256, {}), (0, 256, 2, 1, 4096, 1), [(0, 0, 1, 256, 256, 16928, 0)]),
    ((3, (4096,), 4096, RES, 0, MO, 256, {}), (0, 256, 4, 1, 4096, 1), [(0, 0, 1, 256, 256, 33344, 0)]),
    ((8, (4096, 1024, 1024), 4096, PLAIN, 1, MO, 256, {}), (0, 384, 8, 1, 4096, 1), [(0, 0, 2, 256, 256, 66176, 0)]),
    ((16, (4096, 1024, 1024), 4096, PLAIN, 1, MO, 256, {}), (0, 384, 16, 1, 4096, 1), [(0, 0, 2, 256, 256, 131840, 0)]),
    ((8, (4096, 1024, 1024), 4096, PLAIN, 1, TILED, 256, {}), (0, 384, 8, 0, 4096, 1), [(0, 0, 2, 256, 256, 110976, 0)]),
    ((12, (4096, 1024, 1024), 4096, PLAIN, 0, TILED, 256, {}), (0, 384, 16, 0, 2048, 2), [(0, 0, 2, 256, 256, 90624, 0)]),
    # -- tiles per workgroup: 5 -> 6, 7 -> 8, past 8 the workgroups queue
    ((2, (16416,), 128, PLAIN, 0, MO, 256, {}), (0, 1026, 2, 1, 4096, 1), [(0, 0, 6, 256, 256, 49152, 0)]),
    ((2, (24608,), 128, PLAIN, 0, MO, 256, {}), (0, 1538, 2, 1, 4096, 1), [(0, 0, 8, 256, 256, 65536, 0)]),
    ((3, (33024,), 128, PLAIN, 0, TILED, 256, {}), (0, 2064, 4, 0, 4096, 1), [(0, 0, 8, 258, 258, 78144, 0)]),
    ((2, (12288,), 128, PLAIN, 0, MO, 256, {}), (0, 768, 2, 1, 4096, 1), [(0, 0, 3, 256, 256, 24576, 0)]),
    # -- gated pairs: 2, 3, 4 pairs; past 4 the workgroups queue
    ((4, (4224,), 128, GLU, 1, MO, 256, {}), (0, 264, 4, 1, 4096, 1), [(0, 0, 4, 256, 256, 33344, 0)]),
    ((12, (12288,), 128, GLU, 1, MO, 256, {}), (0, 768, 16, 1, 4096, 1), [(0, 0, 6, 256, 256, 131840, 0)]),
    ((12, (11008,), 4096, GLU, 0, TILED, 256, {}), (0, 688, 16, 0, 2048, 2), [(0, 0, 6, 256, 256, 90624, 0)]),
    ((20, (12416,), 128, GLU, 0, MO, 256, {}), (0, 776, 32, 0, 2048, 1), [(0, 0, 8, 256, 256, 131584, 0)]),
    ((4, (16512,), 128, GLU, 1, MO, 256, {}), (0, 1032, 4, 1, 4096, 1), [(0, 0, 8, 258, 258, 65536, 0)]),
    # -- whole rows (MO, <= 4 rows, K <= 16384; the 150 KiB limit is never the one that binds: 4 rows of 16384 columns are 131136 bytes)
    ((4, (128,), 11008, RES, 0, MO, 256, {}), (0, 8, 4, 2, 4096, 3), [(0, 0, 1, 8, 8, 88128, 0)]),
    ((2, (128,), 16384, RES, 0, MO, 256, {}), (0, 8, 2, 2, 4096, 4), [(0, 0, 1, 8, 8, 65568, 0)]),
    ((4, (128,), 16512, RES, 0, MO, 256, {}), (0, 8, 4, 0, 4096, 5), [(0, 0, 1, 8, 8, 33344, 0)]),
    ((5, (128,), 11008, RES, 0, MO, 256, {}), (0, 8, 8, 0, 4096, 3), [(0, 0, 1, 8, 8, 66176, 0)]),
    # -- K parts, KPM 1 (reachable: Wo / W2 of any model at 9..32 rows)
    ((9, (128,), 4224, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 2), [(2, 1, 2, 4, 8, 131840, 32768), (0, 0, 1, 8, 8, 131840, 0)]),
    ((16, (128,), 12288, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 3), [(3, 1, 3, 3, 9, 131840, 55296), (0, 0, 1, 8, 8, 131840, 0)]),
    ((16, (128,), 16384, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 4), [(4, 1, 4, 2, 8, 131840, 65536), (0, 0, 1, 8, 8, 131840, 0)]),
    ((16, (128,), 24576, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 6), [(6, 1, 6, 2, 12, 131840, 147456), (0, 0, 1, 8, 8, 131840, 0)]),
    ((16, (128,), 32768, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 8), [(8, 1, 8, 1, 8, 131840, 131072), (0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 36864, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 9), [(3, 1, 3, 3, 9, 131840, 55296), (0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 20480, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 5), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 28672, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 7), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((16, (128,), 11008, RES, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 3), [(3, 1, 3, 3, 9, 131840, 55296), (0, 0, 1, 8, 8, 131840, 0)]),
    ((17, (128,), 11008, RES, 0, MO, 256, {}), (0, 8, 32, 0, 2048, 6), [(6, 1, 6, 2, 12, 131584, 294912), (0, 0, 1, 8, 8, 131584, 0)]),
    # (256 tiles: three parts would need 258 workgroups, six likewise; two parts of 128 groups fit exactly)
    ((16, (4096,), 11008, RES, 0, MO, 256, {}), (0, 256, 16, 0, 4096, 3), [(0, 0, 1, 256, 256, 131840, 0)]),
    ((32, (4096,), 11008, RES, 0, MO, 256, {}), (0, 256, 32, 0, 2048, 6), [(2, 1, 2, 128, 256, 131584, 2097152), (0, 0, 1, 256, 256, 131584, 0)]),
    ((32, (4096,), 11008, RES, 0, MO, 256, dict(visible_cus=255)), (0, 256, 32, 0, 2048, 6), [(0, 0, 1, 256, 256, 131584, 0)]),
    # -- K parts, KPM 2: the QKV launch at 17..32 rows is the only one a model reaches on 256 CUs (4 tiles per group)
    ((32, (4096, 1024, 1024), 4096, PLAIN, 0, MO, 256, {}), (0, 384, 32, 0, 2048, 2), [(2, 2, 4, 96, 192, 131584, 3145728), (0, 0, 2, 256, 256, 131584, 0)]),
    ((16, (1024,), 8192, RES, 0, MO, 32, {}), (0, 64, 16, 0, 4096, 2), [(2, 2, 4, 16, 32, 131840, 262144), (0, 0, 2, 32, 32, 131840, 0)]),
    ((32, (1920,), 12288, RES, 0, MO, 64, {}), (0, 120, 32, 0, 2048, 6), [(3, 2, 6, 20, 60, 131584, 1474560), (0, 0, 2, 64, 64, 131584, 0)]),
    ((32, (1024,), 16384, RES, 0, MO, 32, {}), (0, 64, 32, 0, 2048, 8), [(4, 2, 8, 8, 32, 131584, 1048576), (0, 0, 2, 32, 32, 131584, 0)]),
    # -- three or more tiles per workgroup: never K parts
    ((16, (4096,), 8192, RES, 0, MO, 32, {}), (0, 256, 16, 0, 4096, 2), [(0, 0, 8, 32, 32, 131840, 0)]),
    # -- the vetoes and settings
    ((9, (128,), 4224, RES, 0, MO, 256, dict(no_waits=1)), (0, 8, 16, 0, 4096, 2), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 4224, RES, 0, MO, 256, dict(waits_on=0)), (0, 8, 16, 0, 4096, 2), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 4224, RES, 0, MO, 256, dict(kparts_off=1)), (0, 8, 16, 0, 4096, 2), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 4224, RES, 0, MO, 256, dict(kparts_min=3)), (0, 8, 16, 0, 4096, 2), [(0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 12288, RES, 0, MO, 256, dict(kparts_min=3)), (0, 8, 16, 0, 4096, 3), [(3, 1, 3, 3, 9, 131840, 55296), (0, 0, 1, 8, 8, 131840, 0)]),
    ((9, (128,), 4224, GLU, 0, MO, 256, {}), (0, 8, 16, 0, 4096, 2), [(0, 0, 2, 8, 8, 131840, 0)]),
    ((2, (8192,), 128, PLAIN, 0, MO, 256, dict(wgs_per_cu=2)), (0, 512, 2, 1, 4096, 1), [(0, 0, 1, 512, 512, 16928, 0)]),
    ((9, (8192,), 128, PLAIN, 0, MO, 256, dict(wgs_per_cu=2)), (0, 512, 16, 1, 4096, 1), [(0, 0, 2, 256, 256, 131840, 0)]),
]


@pytest.mark.parametrize("facts,want_head,want_tries", TABLE, ids=["T%d-%s-K%d-e%d-n%d-%s-cu%d%s" % (
    f[0], "+".join(map(str, f[1])), f[2], f[3], f[4], "mo" if f[5] else "tiled", f[6], "".join("-%s%d" % kv for kv in f[7].items())) for f, _, _ in TABLE])
def test_plan_table(facts, want_head, want_tries):
    T, rows, K, epi, norm, mo, cus, over = facts
    p = U.plan(T, rows, K, epi, norm, mo, cus, **over)
    assert head(p) == want_head
    assert tries(p) == want_tries


REFUSALS = [
    ("one row", dict(T=1), 1), ("17 rows, tiled", dict(T=17, mo=0), 1), ("33 rows", dict(T=33), 1), ("K not whole supersteps", dict(cols=160), 1),
    ("four sets", dict(nsets=4), 1), ("no set", dict(nsets=0), 1),
    ("norm past one chunk", dict(norm=1, cols=4224), 2), ("norm at 9 rows, tiled", dict(norm=1, T=9, mo=0), 2), ("norm at 17 rows", dict(norm=1, T=17), 2),
    ("gated pair of three sets", dict(epi=GLU, rows=(128, 128, 128)), 3), ("gated pair without W3", dict(epi=GLU, has_w1=0), 3),
    ("a set without rows", dict(rows=(0,), nsets=1), 4), ("24 rows in one of two sets", dict(rows=(128, 24)), 4),
    ("byte offsets past 32 bits", dict(rows=(1 << 20,), cols=65536), 5),
    ("residual behind the norm prologue", dict(epi=RES, norm=1), 6), ("residual behind the norm prologue, tiled", dict(epi=RES, norm=1, mo=0), 6),
    ("tiled gated pair without the norm at 4 rows", dict(epi=GLU, norm=0, mo=0), 6), ("an epilogue the kernel does not have", dict(epi=3), 6),
    ("a norm kind the kernel does not have", dict(norm=2), 6),
]


@pytest.mark.parametrize("why,over,error", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_plan_refuses(why, over, error):
    f = dict(T=4, rows=(128,), cols=256, epi=PLAIN, norm=0, mo=1)
    f.update(over)
    p = U.plan(f.pop("T"), f.pop("rows"), f.pop("cols"), f.pop("epi"), f.pop("norm"), f.pop("mo"), 256, **f)
    assert p["error"] == error and p["tries"] == [] and p["tx"] == 0, (why, p)


def test_plan_accepts_what_sits_next_to_a_refusal():
    for over in (dict(T=2), dict(T=16, mo=0), dict(T=32), dict(norm=1, cols=4096), dict(norm=1, T=8, mo=0), dict(norm=1, T=16), dict(epi=GLU, norm=0),
                 dict(epi=GLU, norm=0, mo=0, T=12), dict(epi=GLU, norm=1, mo=0, T=8), dict(rows=(128, 32))):
        f = dict(T=4, rows=(128,), cols=256, epi=PLAIN, norm=0, mo=1)
        f.update(over)
        assert U.plan(f["T"], f["rows"], f["cols"], f["epi"], f["norm"], f["mo"])["error"] == 0, over


def test_entry_points_check_their_counts():
    L = ia.lib()
    facts, out = (C.c_int * 17)(), (C.c_int * 22)()
    facts[12] = 256
    assert L.ifa_gemm_rows_plan(facts, 16, out, 22) != 0 and L.ifa_gemm_rows_plan(facts, 17, out, 21) != 0
    assert L.ifa_gemm_rows_plan(None, 17, out, 22) != 0
    facts[12] = 0
    assert L.ifa_gemm_rows_plan(facts, 17, out, 22) != 0           # (no CUs)
    rec = (C.c_int * (2 + 8 * 23))()
    assert L.ifa_gemm_rows_launches(rec, 2 + 8 * 23 - 1) != 0 and L.ifa_gemm_rows_launches(None, 2 + 8 * 23) != 0
    assert L.ifa_gemm_rows_launches(rec, len(rec)) == 0                                       # (drains whatever this process launched before)
    assert L.ifa_gemm_rows_launches(rec, len(rec)) == 0 and rec[0] == 0 and rec[1] == 0      # read means cleared
    assert L.ifa_debug_gemm_rows_record(rec, 22, -1) != 0 and L.ifa_debug_gemm_rows_record(None, 23, -1) != 0
    assert len(Wk.GEMM_ROWS_RECORD) == 23 and len(Wk.GEMM_ROWS_FACTS) == 17


def test_launch_record_ring_keeps_the_last_eight_and_survives_the_wrap_of_its_count():
    """the slot index stays in 0 .. 7 and the count of launches since the last read saturates at 2^31 - 1: a process that never reads the
    record (every serving process) can launch for ever"""
    n = len(Wk.GEMM_ROWS_RECORD)
    push = lambda tag, before=-1: ia.check(ia.lib().ifa_debug_gemm_rows_record((C.c_int * n)(*([tag] * n)), n, before))
    Wk.gemm_rows_launches()
    for t in range(1, 4):
        push(t)
    recs, total = Wk.gemm_rows_launches()
    assert total == 3 and [r["T"] for r in recs] == [1, 2, 3] and all(set(r.values()) == {r["T"]} for r in recs)
    for t in range(1, 12):                                   # more than the ring holds: the last eight, oldest first
        push(t)
    recs, total = Wk.gemm_rows_launches()
    assert total == 11 and [r["T"] for r in recs] == list(range(4, 12))
    assert Wk.gemm_rows_launches() == ([], 0)
    top = 2 ** 31 - 1
    push(100, top - 3)                                       # three launches short of the count's top, then across it
    for t in range(101, 120):
        push(t)
    recs, total = Wk.gemm_rows_launches()
    assert total == top and [r["T"] for r in recs] == list(range(112, 120))
    for t in range(1, 3):                                    # and the ring is whole afterwards
        push(t)
    recs, total = Wk.gemm_rows_launches()
    assert total == 2 and [r["T"] for r in recs] == [1, 2]


# ----------------------------------------------------------------------------- faults
def _launch_shapes(group):
    """the distinct launches of the device test's cases of one group, with the plan of each on 256 CUs"""
    seen = {}
    models = [(mc, mc.ns) for mc in U.model_cases(256) if mc.group == group]
    if group == "prompt":                                   # the last pass of every prompt of the device test (the tiled layout: up to 16 rows)
        models = [(U.prompt_model(mo), sorted({U.prompt_passes(T)[-1][1] for T in U.PROMPT_TOKENS if mo or T <= 16})) for mo in (1, 0)]
    for mc, ns in models:
        for n in ns:
            for role, c in mc.launches(n).items():
                over = {} if mc.kparts else dict(no_waits=1)
                seen.setdefault(c.id + ("" if mc.kparts else "-nokparts"), (c, c.plan(256, **over)))
    return list(seen.values())


GROUPS = ("rows", "tiles", "gated", "kdim", "klong", "kparts", "prompt")


@pytest.mark.parametrize("group", GROUPS)
def test_every_fault_is_rejected_with_margin(group):
    smallest = (np.inf, None)
    count = 0
    for c, p in _launch_shapes(group):
        assert p["error"] == 0, c.id
        inp = U.synth_inputs(c, p)
        ref = U.RowsRef(inp)
        good = ref.device_like()
        assert U.violations(good, ref) == 0, c.id
        tb = ref.total_bound(U.F_FLIPS)
        for name, y in ref.faults(p):
            margin = float((np.abs(y - ref.f64) / tb).max())
            assert margin >= U.SENSITIVITY, "%s: '%s' moves no element by %g x its bound (most: %.2f)" % (c.id, name, U.SENSITIVITY, margin)
            bad = ref.device_like(y - ref.f64)
            assert U.violations(bad, ref) > 0, "%s: '%s' passes the check" % (c.id, name)
            with pytest.raises(AssertionError):
                U.check(bad, ref)
            if margin < smallest[0]:
                smallest = (margin, "%s: %s" % (c.id, name))
            count += 1
    print("rows-gemm faults %-6s %5d faults rejected, smallest margin %.1f x bound (%s)" % (group, count, smallest[0], smallest[1]))


@pytest.mark.parametrize("group", GROUPS)
def test_norm_fused_launches_stay_inside_the_flip_term_when_the_scale_moves_one_ulp(group):
    worst = 0
    for c, p in _launch_shapes(group):
        inp = U.synth_inputs(c, p)
        if inp.raw is None:
            continue
        ref = U.RowsRef(inp)
        for X in U.perturbed_inputs(inp):
            Xr = np.ascontiguousarray(X)
            import oracle as o
            ys = [o.gemm_f16x(m.dtype, m.data, m.rows, m.cols, Xr, m.bias) for m in inp.mats]
            if c.epi == GLU:
                out = o.mul(o.act(ys[0], c.act_kind), o.gemm_f16x(inp.w3.dtype, inp.w3.data, inp.w3.rows, inp.w3.cols, Xr, inp.w3.bias))
            else:
                out = np.concatenate(ys, axis=1)
            if ref.exact:
                assert np.array_equal(np.asarray(out).view(np.uint16), ref.orc.view(np.uint16)), c.id      # (the sign family does not move at all)
            else:
                worst = max(worst, U.check(out, ref)[3])
    assert worst <= U.F_FLIPS
