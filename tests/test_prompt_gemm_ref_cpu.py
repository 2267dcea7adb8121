"""CPU-only: the references, layouts and assertions of the prompt-GEMM edge cases (tests/prompt_gemm_util.py), for every shape, format and
seed of its case lists (planned for 256 CUs).

  * the MO layout built in NumPy from the description in csrc/ifa_gemm_rows_mfma.h, decoded back with k_gemm_mid's address arithmetic,
    equals the oracle's dequantisation; rows past the end and the pad of the last quad are zero; the expanded copy of the 64-weight
    formats dequantises, as Q4_B32T1A, to the same values;
  * an output as a correct device gives it passes check_exact; every systematic fault of Ref.mutations moves the float64 output of at
    least one element by >= SENSITIVITY x its bound, and check_exact rejects the oracle's output shifted by that fault;
  * check_sentinel sees a store one row or one column outside the output."""
import numpy as np
import pytest

import oracle as o
from inferflow_amd import dtypes as dt
from tests import prompt_gemm_util as U

CASES = U.mid_cases(256) + U.big_cases(256)
LAYOUT_SHAPES = [(r, c) for r in (16, 24, 144) for c in (128, 640, 1024)]


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize("dtype", U.NIBBLE_FORMATS, ids=lambda d: dt.name(d).lower())
def test_mo_layout_decodes_to_the_oracles_values(dtype):
    for rows, cols in LAYOUT_SHAPES:
        data = U.quantized(dtype, rows, cols, 100 + rows + cols)
        mo = U.mo_build_np(dtype, data, rows, cols)
        assert mo.size == U.mo_bytes(rows, cols)
        want = o.dequantize(dtype, data, cols)
        got = U.mo_decode_np(mo, rows, cols)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), (dt.name(dtype), rows, cols)
        # rows past the end, and the words of the supersteps the last quad does not have
        nsup, ntile = cols // 128, (rows + 15) // 16
        m = mo.reshape(ntile, nsup + (nsup + 3) // 4, 64, 16)
        for r in range(rows % 16 or 16, 16):
            assert not m[-1, :, r::16, :].any()
        if nsup % 4:
            assert not m[:, -1, :, 4 * (nsup % 4):].any()
        assert m[:, :nsup].any() and m[:, nsup:].any()
    if dtype in (dt.Q4_B32T1A, dt.Q4_B32T1B):       # the code bytes of these formats are the reference block's own
        nib, words = U._nibble_bytes_and_words(dtype, data, cols)
        raw = data.reshape(rows, cols // 32, 20)
        assert np.array_equal(nib, raw[:, :, 4:]) and np.array_equal(words, raw[:, :, :4])


@pytest.mark.parametrize("dtype", (dt.Q4_B64T1, dt.Q3H_B64T1), ids=lambda d: dt.name(d).lower())
def test_expanded_copy_has_the_same_values(dtype):
    for rows, cols in LAYOUT_SHAPES:
        data = U.quantized(dtype, rows, cols, 200 + rows + cols)
        x32 = U.expand_b64_np(dtype, data, rows, cols)
        assert x32.shape == (rows, cols // 32 * 20)
        got = o.dequantize(dt.Q4_B32T1A, x32, cols)
        assert np.array_equal(got.view(np.uint16), o.dequantize(dtype, data, cols).view(np.uint16))


def test_words_and_codes_give_the_dequantised_halves():
    """the decomposition the (base, scale) mutations use: half(q x scale + base) is the oracle's value"""
    for dtype in U.NIBBLE_FORMATS:
        data = U.quantized(dtype, 16, 256, 300)
        q, base, scale = U.codes_and_words(dtype, data, 256)
        w = (q.astype(np.float32) * np.repeat(scale, 32, axis=1) + np.repeat(base, 32, axis=1)).astype(np.float16)
        assert np.array_equal(w.view(np.uint16), o.dequantize(dtype, data, 256).view(np.uint16))


def test_part_steps_and_tail_columns():
    assert U.part_steps(10, 2) == [(0, 5), (5, 5)]                       # the second part starts on an odd half
    assert U.part_steps(18, 4) == [(0, 4), (4, 5), (9, 4), (13, 5)]
    assert [n for _, n in U.part_steps(34, 8)] == [4, 4, 4, 5, 4, 4, 4, 5]
    assert U.tail_columns(640, 2) == [(256, 320), (576, 640)]
    assert list(U.oracle_rows(1)) == [0] and list(U.oracle_rows(9)) == [0, 7, 8]
    assert list(U.oracle_rows(129))[-2:] == [127, 128] and len(U.oracle_rows(129)) == 33


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_assertions_reject_every_fault(case):
    parts = case.parts(256)
    ref = U.Ref(U.Inputs(case, parts))
    assert ref.d_ref > 0 or case.T * case.N < 64
    med, worst = U.check_exact(ref.device_like(), ref)
    assert worst <= 1.0
    seen = 0
    for name, mut in ref.mutations(parts):
        delta = mut - ref.f64
        moved = float((np.abs(delta) / ref.bound).max())
        assert moved >= U.SENSITIVITY, "%s: '%s' moves no element by %g x its bound (most: %.3g)" % (case.id, name, U.SENSITIVITY, moved)
        with pytest.raises(AssertionError):
            U.check_exact(ref.device_like(delta), ref)
        seen += 1
    assert seen >= 4, (case.id, seen)


def test_sentinel_check_sees_a_store_outside():
    T, n, ld = 5, 16, 32
    f = U.sentinel_frame(T, n, ld)
    g = f.copy()
    g[:T, :n] = 0
    U.check_sentinel(g, T, n, ld)
    for pos in ((T, 0), (0, n), (T + U.PAD_ROWS - 1, ld - 1), (T - 1, n)):
        h = g.copy()
        h[pos] = 0
        with pytest.raises(AssertionError):
            U.check_sentinel(h, T, n, ld)
    assert len(np.unique(f[0, :8])) == 8
