"""CPU-only: the reference, the inputs and the assertions of the decode-GEMV edge tests (tests/decode_gemv_util.py) do what the GPU test
(tests/test_gpu_decode_gemv_edges.py) relies on, for every format and every column edge it walks:

  * the block decomposition the mutations are expressed on adds up to the oracle's own float64 sum;
  * every systematic fault -- a weight block dropped, doubled or paired with another block's activation (every block of the last round of
    the lanes and a sample of the others), the zero-point term omitted, the residual dropped or doubled, rows finished with the next row's
    sum -- moves the float64 output of at least one row by >= 5 x the bound the GPU test applies (the exact bound; on prologue launches
    the bound with the F code flips the GPU test allows), and check() rejects the oracle's output shifted by that fault;
  * the unmutated oracle output passes;
  * the sign family is immune to the last bit of the norm, and on the dense / tail families a one-ulp change of the norm's scale leaves
    the share of rows that need the flip term within the cap the GPU test applies.
Weights: N(0, 0.06) like the GPU test's models (their own come from the device's generator), 64 rows."""
import numpy as np
import pytest

import oracle as o
from inferflow_amd import dtypes as dt
from tests import decode_gemv_util as U

ROWS = 64
F_GPU = 1          # the flips the GPU test allows a prologue row (tests/test_gpu_decode_gemv_edges.py: F)


def _mat(dtype, cols, seed, rows=ROWS, bias=False):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.06, (rows, cols)).astype(np.float16)
    b = rng.normal(0, 0.06, rows).astype(np.float16) if bias else None
    return U.Mat(dtype, w if dtype == dt.F16 else o.quantize(dtype, w), rows, cols, bias=b)


WIRING_FORMATS = (dt.Q4_B32T1A, dt.Q3H_B64T1)        # the formats the GPU test walks the wirings with, at the nj 1 and 2 edges


def _launches(dtype, cols, family, seed):
    """the launch shapes a width is walked with: a prologue launch (QKV-like, and the gated pair) and a plain one with a residual; at the
    widths of the wirings also their epilogues: a plain activation (SiLU behind the RMS norm, GELU behind the std norm), the
    attn_out_scale / ffn_out_scale factors in front of the residual, Wo without a residual, W2 with two, a gated pair with biases"""
    x = U.make_input(family, cols, dtype, seed)
    ones = np.ones(cols, np.float16)
    xn = o.rmsnorm(x.reshape(1, -1), ones)[0]
    exact = U.norm_exact(family, 0, ones)
    rng = np.random.default_rng(seed + 1)
    res, res2 = rng.normal(0, 1, ROWS).astype(np.float16), rng.normal(0, 1, ROWS).astype(np.float16)
    mk = lambda m: U._product(m, xn)
    out = [U.Launch("plain+residual", [mk(_mat(dtype, cols, seed + 2, bias=True))], U.EPI_RESIDUAL, True, res=res),
           U.Launch("prologue", [mk(_mat(dtype, cols, seed + 3))], U.EPI_PLAIN, exact),
           U.Launch("gated", [mk(_mat(dtype, cols, seed + 4)), mk(_mat(dtype, cols, seed + 5))], U.EPI_GLU, exact)]
    if dtype in WIRING_FORMATS and cols in [c for nj in (1, 2) for c in U.nj_edges(dtype, nj)]:
        xs = o.stdnorm(x.reshape(1, -1), *U.std_norm_affine(cols))[0]
        out += [U.Launch("act", [mk(_mat(dtype, cols, seed + 6))], U.EPI_ACT, exact),
                U.Launch("std norm, gelu", [U._product(_mat(dtype, cols, seed + 7), xs)], U.EPI_ACT, False, act_kind=1),
                U.Launch("std norm, plain", [U._product(_mat(dtype, cols, seed + 8), xs)], U.EPI_PLAIN, False),
                U.Launch("scale 0.25 + residual", [mk(_mat(dtype, cols, seed + 9))], U.EPI_RESIDUAL, True, res=res, pre=0.25),
                U.Launch("scale 0.5 + residual", [mk(_mat(dtype, cols, seed + 10))], U.EPI_RESIDUAL, True, res=res, pre=0.5),
                U.Launch("no residual", [mk(_mat(dtype, cols, seed + 11))], U.EPI_PLAIN, True),
                U.Launch("two residuals", [mk(_mat(dtype, cols, seed + 12))], U.EPI_RESIDUAL, True, res=res, res2=res2),
                U.Launch("gated + biases", [mk(_mat(dtype, cols, seed + 13, bias=True)), mk(_mat(dtype, cols, seed + 14, bias=True))], U.EPI_GLU, exact)]
    return out


def _widths(dtype):
    """(cols, seed of the layer input) of every width the GPU test walks: the wide, long, rows and wiring widths with seed_of(cols), and
    the 256 columns the QKV and W1 / W3 launches of the long models see with SEED_LONG"""
    if dtype in U.INT8_FORMATS:
        w = {c for c, _ in U.wide_edges(dtype)} | {e[0] for e in U.long_edges(dtype)} | {c for nj in (1, 2) for c in U.nj_edges(dtype, nj)}
    else:
        w = set(U.f16x_wide_edges(dtype)) | set(U.f16x_long_edges(dtype))
    return [(c, U.seed_of(c)) for c in sorted(w)] + [(256, U.SEED_LONG)]


ALL = [(d, f) for d in U.INT8_FORMATS + U.F16X_FORMATS for f in ("dense", "sign", "tail")]


@pytest.mark.parametrize("dtype,family", ALL, ids=["%s-%s" % (dt.name(d), f) for d, f in ALL])
def test_every_systematic_fault_is_rejected(dtype, family):
    worst = (np.inf, None)
    for cols, seed in _widths(dtype):
        blocks = U.probed_blocks(dtype, cols)
        if family == "tail":                               # (the other blocks see a zero activation: nothing to lose)
            lo, hi = U.last_round_cols(dtype, cols)
            blocks = [j for j in blocks if lo <= j * U.capacity(dtype) < hi]
        for L in _launches(dtype, cols, family, seed):
            if cols > 8192 and L.name != "plain+residual":
                continue                                   # (normalised / gated inputs end at 8192 columns)
            B = L.products[0].blocks()
            assert np.abs(B.sum(axis=1) - (L.products[0].y64 - (0 if L.products[0].mat.bias is None else L.products[0].mat.bias.astype(np.float64)))).max() \
                <= 1e-9 * max(np.abs(B).sum(axis=1).max(), 1e-30), ("the blocks do not add up to the oracle's float64 sum", cols, L.name)
            F = 0 if L.exact else F_GPU
            U.check(L.orc.astype(np.float16), L, F)        # the oracle itself passes
            tol = L.bound + L.flip_extra(F)
            for name, mut in L.mutations(blocks):
                moved = float((np.abs(mut - L.f64) / tol).max())
                if moved < worst[0]:
                    worst = (moved, (cols, L.name, name))
                assert moved >= U.SENSITIVITY, "%s, %d columns, %s: %s moves the float64 output by %.2f x the bound only" % (dt.name(dtype), cols, L.name, name, moved)
                bad = o.f2h((L.orc + (mut - L.f64)).astype(np.float32))
                assert U.violations(bad, L, F) > 0, (cols, L.name, name)
                if name.startswith("rows of product 0"):      # (one fault per launch through check() itself: it raises where violations() counts)
                    with pytest.raises(AssertionError):
                        U.check(bad, L, F)
    print("decode-gemv-ref %-10s %-5s least sensitive fault %.1f x the bound: %s" % (dt.name(dtype), family, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", U.INT8_FORMATS + U.F16X_FORMATS, ids=[dt.name(d) for d in U.INT8_FORMATS + U.F16X_FORMATS])
def test_a_last_bit_of_the_norm(dtype):
    """one fp32 ulp of the RMS scale either way, at the widths and seeds of the GPU test's prologue launches.  sign: the same F16 vector,
    hence the same Q8 image.  dense / tail: the quantised
    images differ in a few codes; the rows of a prologue launch computed from the perturbed image that leave the exact bound of the
    unperturbed reference stay within FLIP_ROWS_MAX, and none needs more than F_GPU flips"""
    wide = [c for c, _ in U.wide_edges(dtype)] if dtype in U.INT8_FORMATS else U.f16x_wide_edges(dtype)
    for cols, seed in [(c, U.seed_of(c)) for c in wide] + [(256, U.SEED_LONG)]:
        x = U.make_input("sign", cols, dtype, seed)
        lo, mid, hi = U.perturbed_norms(x)
        assert np.array_equal(lo.view(np.uint16), mid.view(np.uint16)) and np.array_equal(hi.view(np.uint16), mid.view(np.uint16)), cols
        assert np.array_equal(np.abs(mid.astype(np.float32)), np.ones(cols, np.float32))
        codes, xs = U.q8_parts(U.q8_image(mid), cols)
        assert np.array_equal(np.abs(codes), np.full_like(codes, 127)) and np.unique(xs).size == 1
        assert np.array_equal(o.rmsnorm(x.reshape(1, -1), np.ones(cols, np.float16))[0].view(np.uint16), mid.view(np.uint16))
        for family in ("dense", "tail"):
            x = U.make_input(family, cols, dtype, seed)                             # (the seeds of the GPU test)
            lo, mid, hi = U.perturbed_norms(x)
            m = _mat(dtype, cols, 7, rows=256)
            L = U.Launch("prologue", [U._product(m, mid)], U.EPI_PLAIN, False)
            for other in (lo, hi):
                out = U._product(m, other).y16
                U.check(out, L, F_GPU)
