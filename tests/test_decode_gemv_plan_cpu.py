"""CPU-only checks of the decode GEMV launch plan (csrc/ifa_decode_gemv_plan.h) through the host-only entry point ifa_decode_gemv_plan:
which kernel a launch runs (k_dec_gemv, k_dec_gemv_long, k_dec_gemv_h), with how many blocks per lane (nj), register chunks (nchunk,
njl), rows per wave, threads, prologue waves, grid, passes and LDS bytes, and what it refuses.  Tables only; the expected values are
written out by hand from the rules of the launchers, not computed:

  nj     = ceil(blocks / 64), blocks = cols / capacity (32: Q4_B32T1A/B, Q8_B32T2; 64: Q4_B64T1, Q3H_B64T1, Q3H_NATIVE, Q5_B64T1, Q6_B64T1)
  MAXNJ  = 8 (Q4_B32T1A/B), 6 (Q8_B32T2), 4 (the B64 formats); past it nchunk = ceil(nj / MAXNJ), njl = ceil(nj / nchunk), k_dec_gemv_long
  LDS    = cols rounded up to 16 + 8 * (cols / 32), up to 16, + 528, up to 16, + 2 * cols + 16  (fp16 activations: 2 * cols up to 16 + 528)
Under the 32768-column limit no format reaches 4 chunks (that needs more than 3 * MAXNJ * 64 blocks: 49152 columns of Q4_B32T1, 36864 of
Q8_B32T2, 49152 of a B64 format) and only Q8_B32T2 reaches 3 (past 24576 columns): the "more than 4 chunks" refusal of the launcher
cannot be met before the column limit, and no launch packs more than 0xFFFF blocks per row (1024 at most)."""
import pytest

from inferflow_amd import dtypes as dt, worker as W

PLAIN, RESIDUAL, GLU, ACT, MOE_ACC = 0, 1, 2, 3, 4
Q3H_NATIVE = 99            # internal id of csrc/ifa_dtype.h (option q3h_native)
OK, E_DTYPE, E_COLS, E_LONG, E_NJ, E_PACKED, E_NOKERNEL = 0, 1, 2, 3, 4, 5, 6
B32_8 = (dt.Q4_B32T1A, dt.Q4_B32T1B)
B64 = (dt.Q4_B64T1, dt.Q3H_B64T1, Q3H_NATIVE, dt.Q5_B64T1, dt.Q6_B64T1)


def plan(dtype, epi, norm, cols, rows=4096, cus=256, **kw):
    return W.gemv_plan(dtype, epi, norm, cols, rows, cus, **kw)


# (cols, kind, nj, nchunk, njl) of a W2-type launch (RESIDUAL, no norm): every multiple of 64 blocks, one block less, one block more
Q4_COLS = [(32, "classic", 1, 1, 1), (2016, "classic", 1, 1, 1), (2048, "classic", 1, 1, 1), (2080, "classic", 2, 1, 2),
           (4064, "classic", 2, 1, 2), (4096, "classic", 2, 1, 2), (4128, "classic", 3, 1, 3),
           (6112, "classic", 3, 1, 3), (6144, "classic", 3, 1, 3), (6176, "classic", 4, 1, 4),
           (8160, "classic", 4, 1, 4), (8192, "classic", 4, 1, 4), (8224, "classic", 5, 1, 5),
           (10208, "classic", 5, 1, 5), (10240, "classic", 5, 1, 5), (10272, "classic", 6, 1, 6),
           (12256, "classic", 6, 1, 6), (12288, "classic", 6, 1, 6), (12320, "classic", 7, 1, 7),
           (14304, "classic", 7, 1, 7), (14336, "classic", 7, 1, 7), (14368, "classic", 8, 1, 8),
           (16352, "classic", 8, 1, 8), (16384, "classic", 8, 1, 8),
           # the long kernel from MAXNJ * 64 blocks + 1 on: always two chunks up to 32768 columns
           (16416, "long", 9, 2, 5), (18432, "long", 9, 2, 5), (18464, "long", 10, 2, 5), (20480, "long", 10, 2, 5), (20512, "long", 11, 2, 6),
           (24576, "long", 12, 2, 6), (24608, "long", 13, 2, 7), (28672, "long", 14, 2, 7), (28704, "long", 15, 2, 8),
           (32736, "long", 16, 2, 8), (32768, "long", 16, 2, 8)]
Q8_COLS = [(32, "classic", 1, 1, 1), (2016, "classic", 1, 1, 1), (2048, "classic", 1, 1, 1), (2080, "classic", 2, 1, 2),
           (4064, "classic", 2, 1, 2), (4096, "classic", 2, 1, 2), (4128, "classic", 3, 1, 3),
           (6112, "classic", 3, 1, 3), (6144, "classic", 3, 1, 3), (6176, "classic", 4, 1, 4),
           (8160, "classic", 4, 1, 4), (8192, "classic", 4, 1, 4), (8224, "classic", 5, 1, 5),
           (10208, "classic", 5, 1, 5), (10240, "classic", 5, 1, 5), (10272, "classic", 6, 1, 6),
           (12256, "classic", 6, 1, 6), (12288, "classic", 6, 1, 6),
           (12320, "long", 7, 2, 4), (14336, "long", 7, 2, 4), (14368, "long", 8, 2, 4), (16384, "long", 8, 2, 4), (16416, "long", 9, 2, 5),
           (20480, "long", 10, 2, 5), (20512, "long", 11, 2, 6), (24544, "long", 12, 2, 6), (24576, "long", 12, 2, 6),
           # two chunks -> three past 2 * MAXNJ * 64 blocks
           (24608, "long", 13, 3, 5), (28672, "long", 14, 3, 5), (30720, "long", 15, 3, 5), (30752, "long", 16, 3, 6), (32768, "long", 16, 3, 6)]
B64_COLS = [(64, "classic", 1, 1, 1), (4032, "classic", 1, 1, 1), (4096, "classic", 1, 1, 1), (4160, "classic", 2, 1, 2),
            (8128, "classic", 2, 1, 2), (8192, "classic", 2, 1, 2), (8256, "classic", 3, 1, 3),
            (12224, "classic", 3, 1, 3), (12288, "classic", 3, 1, 3), (12352, "classic", 4, 1, 4),
            (16320, "classic", 4, 1, 4), (16384, "classic", 4, 1, 4),
            (16448, "long", 5, 2, 3), (20480, "long", 5, 2, 3), (20544, "long", 6, 2, 3), (24576, "long", 6, 2, 3), (24640, "long", 7, 2, 4),
            (28672, "long", 7, 2, 4), (28736, "long", 8, 2, 4), (32704, "long", 8, 2, 4), (32768, "long", 8, 2, 4)]
COLS = [(d, row) for d in B32_8 for row in Q4_COLS] + [(dt.Q8_B32T2, row) for row in Q8_COLS] + [(d, row) for d in B64 for row in B64_COLS]


@pytest.mark.parametrize("dtype,row", COLS, ids=["%d-%d" % (d, r[0]) for d, r in COLS])
def test_blocks_per_lane_and_the_switch_to_the_long_kernel(dtype, row):
    cols, kind, nj, nchunk, njl = row
    p = plan(dtype, RESIDUAL, 0, cols)
    assert (p["error"], p["kind"], p["nj"], p["nchunk"], p["njl"]) == (OK, kind, nj, nchunk, njl), p
    assert p["threads"] in (512, 1024) and p["rw"] >= 1 and p["grid"] == 256 and p["waves"] == 256 * p["threads"] // 64
    if kind == "long":
        assert (p["threads"], p["np"]) == (512, 0)
    # the same columns without the residual (PLAIN, 0: Wo of a parallel-attention model) take the same kernel
    q = plan(dtype, PLAIN, 0, cols)
    assert (q["error"], q["kind"], q["nj"], q["nchunk"], q["njl"]) == (OK, kind, nj, nchunk, njl), q


REFUSALS = [
    # more than 4 blocks per lane of a normalised or gated input
    ("q4 qkv 8224", dt.Q4_B32T1A, PLAIN, 1, 8224, {}, E_NJ), ("q4 glu 8224", dt.Q4_B32T1A, GLU, 1, 8224, {}, E_NJ),
    ("q4 act no norm 8224", dt.Q4_B32T1A, ACT, 0, 8224, {}, E_NJ), ("q4 glu no norm 8224", dt.Q4_B32T1B, GLU, 0, 8224, {}, E_NJ),
    ("q8 glu 8224", dt.Q8_B32T2, GLU, 1, 8224, {}, E_NJ), ("q8 qkv 8224", dt.Q8_B32T2, PLAIN, 1, 8224, {}, E_NJ),
    ("q4 qkv 8192 fits", dt.Q4_B32T1A, PLAIN, 1, 8192, {}, OK), ("q8 glu 8192 fits", dt.Q8_B32T2, GLU, 1, 8192, {}, OK),
    # a B64 format: 5 blocks per lane are past MAXNJ, and a normalised / gated / pre-quantised input has no long kernel
    ("q3h qkv 16448", dt.Q3H_B64T1, PLAIN, 1, 16448, {}, E_NJ), ("q5 glu 16448", dt.Q5_B64T1, GLU, 1, 16448, {}, E_NJ),
    ("q3h qkv 16384 fits", dt.Q3H_B64T1, PLAIN, 1, 16384, {}, OK),
    ("q4 wo pre-quantised 16416", dt.Q4_B32T1A, RESIDUAL, 2, 16416, {}, E_NJ), ("q4 wo pre-quantised 16384 fits", dt.Q4_B32T1A, RESIDUAL, 2, 16384, {}, OK),
    # more than 32768 columns
    ("q4 32800", dt.Q4_B32T1A, RESIDUAL, 0, 32800, {}, E_LONG), ("q8 32800", dt.Q8_B32T2, RESIDUAL, 0, 32800, {}, E_LONG),
    ("q6 32832", dt.Q6_B64T1, RESIDUAL, 0, 32832, {}, E_LONG), ("q4 65536", dt.Q4_B32T1A, RESIDUAL, 0, 65536, {}, E_LONG),
    ("f16 32776", dt.F16, RESIDUAL, 0, 32776, {}, E_LONG),
    # no columns, or not whole blocks
    ("q4 0", dt.Q4_B32T1A, RESIDUAL, 0, 0, {}, E_COLS), ("q4 48", dt.Q4_B32T1A, RESIDUAL, 0, 48, {}, E_COLS), ("q3h 96", dt.Q3H_B64T1, RESIDUAL, 0, 96, {}, E_COLS),
    ("f16 12", dt.F16, RESIDUAL, 0, 12, {}, E_COLS), ("q4_b16 16 fits", dt.Q4_B16, RESIDUAL, 0, 16, {}, OK),
    ("q8_b32t1 40", dt.Q8_B32T1, RESIDUAL, 0, 40, {}, E_COLS),
    # the grid does not fit the 16-bit half of the packed launch scalar
    ("q4 grid 65536", dt.Q4_B32T1A, RESIDUAL, 0, 4096, dict(rows=10_000_000, cus=65536), E_PACKED),
    ("q4 grid 65535 fits", dt.Q4_B32T1A, RESIDUAL, 0, 4096, dict(rows=10_000_000, cus=65535), OK),
    ("q4 grid 256 x rpw 256", dt.Q4_B32T1A, RESIDUAL, 0, 4096, dict(rows=10_000_000, cus=256, rpw=256), E_PACKED),
    # no such instance
    ("q4 x_add residual", dt.Q4_B32T1A, RESIDUAL, 0, 4096, dict(x_add=1), E_NOKERNEL), ("q4 residual behind a norm", dt.Q4_B32T1A, RESIDUAL, 1, 4096, {}, E_NOKERNEL),
    ("q4 pre-quantised glu", dt.Q4_B32T1A, GLU, 2, 4096, {}, E_NOKERNEL), ("f16 pre-quantised", dt.F16, RESIDUAL, 2, 4096, {}, E_NOKERNEL),
    ("f16 expert epilogue", dt.F16, MOE_ACC, 0, 4096, {}, E_NOKERNEL), ("q4 x_add qkv", dt.Q4_B32T1A, PLAIN, 1, 4096, dict(x_add=1), OK),
    ("f32", dt.F32, RESIDUAL, 0, 4096, {}, E_DTYPE),
]


@pytest.mark.parametrize("name,dtype,epi,norm,cols,kw,error", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, dtype, epi, norm, cols, kw, error):
    p = plan(dtype, epi, norm, cols, **kw)
    assert p["error"] == error, p
    assert (p["kind"] == "none") == (error != OK), p


# Llama-2-7B on 256 CUs (DESIGN.md "Decode GEMV launch plan"): (role, epi, norm, cols, rows) -> nj, threads, np, rw, npass, partial, lds
ROLES_7B = [
    ("q4 qkv", dt.Q4_B32T1A, PLAIN, 1, 4096, 12288, dict(nj=2, threads=1024, np=8, rw=3, waves=4096, npass=1, partial=0, lds=13856)),
    ("q4 wo", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 4096, dict(nj=2, threads=512, np=0, rw=2, waves=2048, npass=1, partial=0, lds=13856)),
    ("q4 w1w3", dt.Q4_B32T1A, GLU, 1, 4096, 11008, dict(nj=2, threads=1024, np=8, rw=3, waves=4096, npass=1, partial=1, lds=13856)),
    ("q4 w2", dt.Q4_B32T1A, RESIDUAL, 0, 11008, 4096, dict(nj=6, threads=512, np=4, rw=2, waves=2048, npass=1, partial=0, lds=36320)),
    ("q4b w1w3", dt.Q4_B32T1B, GLU, 1, 4096, 11008, dict(nj=2, threads=1024, np=8, rw=3, waves=4096, npass=1, partial=1, lds=13856)),
    ("q3h qkv", dt.Q3H_B64T1, PLAIN, 1, 4096, 12288, dict(nj=1, threads=512, np=4, rw=6, waves=2048, npass=1, partial=0, lds=13856)),
    ("q3h wo", dt.Q3H_B64T1, RESIDUAL, 2, 4096, 4096, dict(nj=1, threads=512, np=0, rw=2, waves=2048, npass=1, partial=0, lds=13856)),
    ("q3h w1w3", dt.Q3H_B64T1, GLU, 1, 4096, 11008, dict(nj=1, threads=1024, np=8, rw=3, waves=4096, npass=1, partial=1, lds=13856)),
    ("q3h w2", dt.Q3H_B64T1, RESIDUAL, 0, 11008, 4096, dict(nj=3, threads=512, np=4, rw=2, waves=2048, npass=1, partial=0, lds=36320)),
    ("q3hn w1w3", Q3H_NATIVE, GLU, 1, 4096, 11008, dict(nj=1, threads=1024, np=8, rw=3, waves=4096, npass=1, partial=1, lds=13856)),
    ("q6 w1w3", dt.Q6_B64T1, GLU, 1, 4096, 11008, dict(nj=1, threads=512, np=4, rw=2, waves=2048, npass=3, partial=1, lds=13856)),
    ("q8 qkv", dt.Q8_B32T2, PLAIN, 1, 4096, 12288, dict(nj=2, threads=512, np=4, rw=4, waves=2048, npass=2, partial=1, lds=13856)),
    ("q8 wo", dt.Q8_B32T2, RESIDUAL, 2, 4096, 4096, dict(nj=2, threads=512, np=0, rw=2, waves=2048, npass=1, partial=0, lds=13856)),
    ("q8 w1w3", dt.Q8_B32T2, GLU, 1, 4096, 11008, dict(nj=2, threads=1024, np=8, rw=2, waves=4096, npass=2, partial=1, lds=13856)),
    ("q8 w2", dt.Q8_B32T2, RESIDUAL, 0, 11008, 4096, dict(nj=6, threads=512, np=4, rw=1, waves=2048, npass=2, partial=0, lds=36320)),
    # the long kernel: half the rows of the single-chunk instance of njl blocks, 512 threads, every wave in the prologue
    ("q4 w2 70b", dt.Q4_B32T1A, RESIDUAL, 0, 28672, 8192, dict(kind="long", nj=14, nchunk=2, njl=7, threads=512, np=0, rw=1, waves=2048, npass=4, partial=0, lds=93728)),
    ("q3h w2 34b", dt.Q3H_B64T1, RESIDUAL, 0, 20480, 7168, dict(kind="long", nj=5, nchunk=2, njl=3, threads=512, np=0, rw=1, waves=2048, npass=4, partial=1, lds=67104)),
]


@pytest.mark.parametrize("name,dtype,epi,norm,cols,rows,want", ROLES_7B, ids=[r[0] for r in ROLES_7B])
def test_instances_of_the_llama2_7b_roles(name, dtype, epi, norm, cols, rows, want):
    p = plan(dtype, epi, norm, cols, rows, 256)
    want = dict(dict(kind="classic", grid=256, error=OK), **want)
    assert {k: p[k] for k in want} == want, p


# rows against the waves of the grid, 256 CUs: (name, dtype, epi, norm, cols, rows) -> grid, waves W, rw, npass, partial
ROWS = [
    # Q4 W1 / W3 at 4096 columns: 1024 threads (16 waves per workgroup), 3 row pairs per wave
    ("glu 5 rows", dt.Q4_B32T1A, GLU, 1, 4096, 5, (1, 16, 3, 1, 1)), ("glu 16", dt.Q4_B32T1A, GLU, 1, 4096, 16, (1, 16, 3, 1, 1)),
    ("glu 17", dt.Q4_B32T1A, GLU, 1, 4096, 17, (2, 32, 3, 1, 1)), ("glu 4080", dt.Q4_B32T1A, GLU, 1, 4096, 4080, (255, 4080, 3, 1, 1)),
    ("glu W", dt.Q4_B32T1A, GLU, 1, 4096, 4096, (256, 4096, 3, 1, 1)), ("glu W + 1", dt.Q4_B32T1A, GLU, 1, 4096, 4097, (256, 4096, 3, 1, 1)),
    ("glu RW x W", dt.Q4_B32T1A, GLU, 1, 4096, 12288, (256, 4096, 3, 1, 0)), ("glu RW x W + 1", dt.Q4_B32T1A, GLU, 1, 4096, 12289, (256, 4096, 3, 2, 1)),
    ("glu 2 RW x W", dt.Q4_B32T1A, GLU, 1, 4096, 24576, (256, 4096, 3, 2, 0)),
    # Q4 Wo at 4096 columns, pre-quantised input: 512 threads, 2 rows per wave
    ("wo W", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 2048, (256, 2048, 2, 1, 1)), ("wo W + 1", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 2049, (256, 2048, 2, 1, 1)),
    ("wo RW x W", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 4096, (256, 2048, 2, 1, 0)), ("wo RW x W + 1", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 4097, (256, 2048, 2, 2, 1)),
    # Q3H W1 / W3 at 2048 columns (one block per lane on half the lanes): 1024 threads, 3 row pairs
    ("q3h glu W", dt.Q3H_B64T1, GLU, 1, 2048, 4096, (256, 4096, 3, 1, 1)), ("q3h glu RW x W + 1", dt.Q3H_B64T1, GLU, 1, 2048, 12289, (256, 4096, 3, 2, 1)),
    # Q8_B32T2 W1 / W3 at 2048 columns: 512 threads, 72 / (2 x 1 x 9) = 4 row pairs
    ("q8 glu W", dt.Q8_B32T2, GLU, 1, 2048, 2048, (256, 2048, 4, 1, 1)), ("q8 glu W + 1", dt.Q8_B32T2, GLU, 1, 2048, 2049, (256, 2048, 4, 1, 1)),
    ("q8 glu RW x W", dt.Q8_B32T2, GLU, 1, 2048, 8192, (256, 2048, 4, 1, 0)), ("q8 glu RW x W + 1", dt.Q8_B32T2, GLU, 1, 2048, 8193, (256, 2048, 4, 2, 1)),
    # two workgroups per CU (option rpw_* = 2)
    ("wo rpw 2", dt.Q4_B32T1A, RESIDUAL, 2, 4096, 4096, (512, 4096, 2, 1, 1), dict(rpw=2)),
    # the fp16-activation kernel: two workgroups per CU, 2 rows per wave
    ("f16 4096 rows", dt.F16, RESIDUAL, 0, 256, 4096, (256, 2048, 2, 1, 0)), ("f16 8193 rows", dt.F16, RESIDUAL, 0, 256, 8193, (512, 4096, 2, 2, 1)),
    ("f16 3 rows", dt.F16, PLAIN, 1, 256, 3, (1, 8, 2, 1, 1)),
]


@pytest.mark.parametrize("case", ROWS, ids=[r[0] for r in ROWS])
def test_passes_and_the_partial_last_pass(case):
    name, dtype, epi, norm, cols, rows, want = case[:7]
    p = plan(dtype, epi, norm, cols, rows, 256, **(case[7] if len(case) > 7 else {}))
    assert p["error"] == OK, p
    assert (p["grid"], p["waves"], p["rw"], p["npass"], p["partial"]) == want, p


# the fp16-activation kernel: lane-loop rounds (F16: 256 chunks of 8 values per round; block formats: 64 blocks), LDS bytes
F16X = [
    (dt.F16, 8, 1, 544), (dt.F16, 2040, 1, 4608), (dt.F16, 2048, 1, 4624), (dt.F16, 2056, 2, 4640), (dt.F16, 4096, 2, 8720), (dt.F16, 4104, 3, 8736),
    (dt.F16, 8192, 4, 16912), (dt.F16, 8200, 5, 16928), (dt.F16, 32768, 16, 66064),
    (dt.Q8_B32T1, 2048, 1, 4624), (dt.Q8_B32T1, 2080, 2, 4688), (dt.Q5_B32T1, 8192, 4, 16912), (dt.Q5_B32T1, 8224, 5, 16976),
    (dt.Q4_B16, 1024, 1, 2576), (dt.Q4_B16, 1040, 2, 2608), (dt.Q3_B32T1A, 16384, 8, 33296), (dt.Q2_B32T1B, 32768, 16, 66064),
]


@pytest.mark.parametrize("dtype,cols,nj,lds", F16X, ids=["%d-%d" % (d, c) for d, c, _, _ in F16X])
def test_fp16_activation_kernel(dtype, cols, nj, lds):
    for epi, norm in ((RESIDUAL, 0), (PLAIN, 1), (GLU, 1), (ACT, 0)):
        p = plan(dtype, epi, norm, cols, 4096, 256)
        assert (p["error"], p["kind"], p["nj"], p["lds"], p["rw"], p["threads"], p["np"], p["nchunk"], p["njl"]) == (OK, "f16x", nj, lds, 2, 512, 0, 0, 0), p


def test_argument_checks_and_exports():
    import ctypes as C
    import inferflow_amd as ia
    L = ia.lib()
    facts = (C.c_int * 8)(dt.Q4_B32T1A, RESIDUAL, 0, 0, 4096, 4096, 256, 0)
    out = (C.c_int * 13)()
    assert L.ifa_decode_gemv_plan(facts, 7, out, 13) != 0
    assert L.ifa_decode_gemv_plan(facts, 8, out, 12) != 0
    assert L.ifa_decode_gemv_plan(None, 8, out, 13) != 0
    assert L.ifa_decode_gemv_plan(facts, 8, out, 13) == 0 and out[0] == 1 and out[1] == 2
    facts[6] = 0
    assert L.ifa_decode_gemv_plan(facts, 8, out, 13) != 0          # no CUs
    for name in ("ifa_decode_gemv_plan", "ifa_model_gemv_plan"):
        assert name in open(__file__.replace("tests/test_decode_gemv_plan_cpu.py", "include/inferflow_amd.h")).read()
        assert hasattr(L, name)
