"""-m gpu: the logit-processor ops (csrc/ifa_logit_adjust.hip) against a float32 numpy restatement of their five steps, F16 output
bit for bit; the two state kernels against a numpy histogram."""
import numpy as np
import pytest

import torch

import inferflow_amd  # noqa: F401
from inferflow_amd import worker as W
from tests.logit_adjust_util import PROMPT_BIT, restate

pytestmark = pytest.mark.gpu

# {rep, freq, pres} per slot: neutral, every rep of the issue, freq and pres of both signs
PARAMS = np.array([[1.0, 0.0, 0.0], [1.3, 0.5, -0.25], [0.5, -0.7, 1.0], [1.3, 0.0, 0.0], [1.0, 2.0, -2.0], [0.5, 0.0, 0.75], [1.0, -0.125, 0.0]], np.float32)
SLOTS = len(PARAMS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(V, stride, rows_avail, seed):
    rng = np.random.default_rng(seed)
    buf = np.zeros((rows_avail, stride), np.float16)
    buf[:, :V] = (rng.normal(0, 8, (rows_avail, V))).astype(np.float16)
    special = np.array([0.0, -0.0, 65504.0, -65504.0, np.nan, -np.inf, np.inf, 60000.0, 1.0, -1.0], np.float16)
    for r in range(rows_avail):                      # the special values at ids that move with the row (every one meets several slots)
        for i, v in enumerate(special):
            buf[r, (r * 3 + i * 5) % V] = v
    state = rng.choice(np.array([0, 1, 7], np.uint32), (SLOTS, V)) | np.where(rng.random((SLOTS, V)) < 0.4, PROMPT_BIT, np.uint32(0))
    state = state.astype(np.uint32)
    bias = np.zeros((SLOTS, V), np.float32)
    pick = rng.random((SLOTS, V))
    bias[pick < 0.06] = 5.0
    bias[(pick >= 0.06) & (pick < 0.12)] = -100.0
    bias[(pick >= 0.12) & (pick < 0.18)] = -np.inf
    bias[(pick >= 0.18) & (pick < 0.22)] = 100.0
    return buf, state, bias


def _vector_rows(V, stride, row_idx, slots):
    """the output rows that take the 16-byte path: input, output, state and bias row all start on a 16-byte boundary (the buffers do)"""
    return [r for r in range(len(slots)) if (int(row_idx[r]) * stride) % 8 == 0 and (r * V) % 8 == 0 and (int(slots[r]) * V) % 4 == 0]


# Which path a shape takes.  Id by id (a base off a 16-byte boundary): V = 1, 63, 1003, and every row of 4096 + 5 but output row 0 on
# slot 0 / 4.  The 16-byte body: 1000 (125 vectors, one workgroup, no tail), 4096 (two workgroups, no tail), 4100 / 4128 (two
# workgroups + a tail of 4; odd output rows id by id), 4096 + 5 / 4128 (row 0 with slot_step 4: two workgroups + a tail of 5),
# 32000 (a real vocabulary: 16 workgroups, the last one's threads 160.. idle).
@pytest.mark.parametrize("slot_step,slot0", [(5, 3), (4, 0)])      # (5r + 3) % 7: permuted, 5 and 7 coprime; (4r) % 7: 0, 4, 1, 5 ...
@pytest.mark.parametrize("rows", [1, 2, 9])
@pytest.mark.parametrize("V,stride", [(1, 1), (63, 63), (1000, 1000), (1003, 1003), (4096 + 5, 4128), (4096, 4096), (4100, 4128), (32000, 32000)])
def test_adjust_rows_bit_exact(V, stride, rows, slot_step, slot0):
    rows_avail = rows + 2
    buf, state, bias = _inputs(V, stride, rows_avail, seed=V * 16 + rows)
    row_idx = np.array([(3 * r + 1) % rows_avail for r in range(rows)], np.int32)
    if rows > 1:
        row_idx[-1] = row_idx[0]                       # a repeated index
    slots = np.array([(slot_step * r + slot0) % SLOTS for r in range(rows)], np.int32)
    vec = _vector_rows(V, stride, row_idx, slots)
    if V in (1000, 4096, 32000):
        assert len(vec) == rows                        # (the production shapes: every row on the 16-byte path)
    if V in (1, 63, 1003):
        assert not vec
    if V in (4096 + 5, 4100) and slot_step == 4:
        assert 0 in vec                                # (the 16-byte body across two workgroups + the n % 8 tail)
    lg_full = _dev(buf)
    lg = lg_full[:, :V]
    out = W.logit_adjust_rows(lg, _dev(slots), _dev(state.view(np.int32)), _dev(bias), _dev(PARAMS), row_idx=_dev(row_idx))
    again = W.logit_adjust_rows(lg, _dev(slots), _dev(state.view(np.int32)), _dev(bias), _dev(PARAMS), row_idx=_dev(row_idx))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert got.shape == (rows, V)
    assert np.array_equal(got, again.cpu().numpy().view(np.uint16))              # run to run
    assert np.array_equal(lg_full.cpu().numpy().view(np.uint16), buf.view(np.uint16))      # pure: the input is untouched
    for r in range(rows):
        want = restate(buf[row_idx[r], :V], state[slots[r]], bias[slots[r]], PARAMS[slots[r]])
        bad = np.nonzero(got[r] != want)[0]
        assert bad.size == 0, (r, bad[:8], got[r][bad[:8]], want[bad[:8]])
    # identity row order (row_idx = NULL)
    ident = W.logit_adjust_rows(lg, _dev(slots), _dev(state.view(np.int32)), _dev(bias), _dev(PARAMS)).cpu().numpy().view(np.uint16)
    for r in range(rows):
        assert np.array_equal(ident[r], restate(buf[r, :V], state[slots[r]], bias[slots[r]], PARAMS[slots[r]])), r


def test_named_cases():
    """the cases the arithmetic is pinned by, one id each: values worked out by hand from the five steps"""
    V = 16
    x = np.zeros((1, V), np.float16)
    state = np.zeros((1, V), np.uint32)
    bias = np.zeros((1, V), np.float32)
    p = np.array([[1.3, 0.5, 0.25]], np.float32)
    x[0, 0] = 60000.0; bias[0, 0] = 100.0                                  # 60100: inside the range, rounds to 60096 (spacing 32)
    x[0, 10] = 65504.0; bias[0, 10] = 100.0                                # clamp: 65604 -> 65504
    x[0, 11] = -65504.0; bias[0, 11] = -100.0                              # clamp: -65604 -> -65504
    x[0, 12] = 60000.0; bias[0, 12] = 100.0; state[0, 12] = 2 | PROMPT_BIT  # 60000 / 1.3 - 1.25 + 100
    x[0, 1] = np.nan; state[0, 1] = 3                                      # NaN stays NaN
    x[0, 2] = -np.inf; state[0, 2] = PROMPT_BIT                            # -inf * rep = -inf -> clamped: -65504
    x[0, 3] = 2.0; state[0, 3] = PROMPT_BIT                                # prompt only: 2 / 1.3, no freq / pres
    x[0, 4] = -2.0; state[0, 4] = 2                                        # generated twice: -2 * 1.3 - (0.5 * 2 + 0.25)
    x[0, 5] = 7.0; bias[0, 5] = -np.inf                                    # banned
    x[0, 6] = 3.0                                                          # never seen: untouched
    x[0, 7] = 1.0; bias[0, 7] = 5.0
    x[0, 8] = 1.0; bias[0, 8] = -100.0
    x[0, 9] = np.nan; bias[0, 9] = -np.inf                                 # the ban wins over NaN
    out = W.logit_adjust_rows(_dev(x), _dev(np.zeros(1, np.int32)), _dev(state.view(np.int32)), _dev(bias), _dev(p)).cpu().numpy()
    f32 = np.float32
    assert out[0, 0] == 60096.0
    assert out[0, 10] == 65504.0 and out[0, 11] == -65504.0
    assert out[0, 12] == np.float16(f32(60000.0) / f32(1.3) - (f32(0.5) * f32(2.0) + f32(0.25)) + f32(100.0))
    assert np.isnan(out[0, 1]) and out.view(np.uint16)[0, 1] == 0x7E00
    assert out[0, 2] == -65504.0
    assert out[0, 3] == np.float16(f32(2.0) / f32(1.3))
    assert out[0, 4] == np.float16(f32(-2.0) * f32(1.3) - (f32(0.5) * f32(2.0) + f32(0.25)))
    assert out[0, 5] == -np.inf
    assert out[0, 6] == 3.0 and out[0, 7] == 6.0 and out[0, 8] == -99.0
    assert out[0, 9] == -np.inf
    assert np.array_equal(out.view(np.uint16), restate(x[0], state[0], bias[0], p[0])[None, :])


@pytest.mark.parametrize("V", [63, 1000, 4096 + 5])
def test_neutral_parameters_reproduce_the_input_bits(V):
    rng = np.random.default_rng(V)
    x = rng.normal(0, 8, (3, V)).astype(np.float16)
    x[:, 0] = 0.0; x[:, 1] = 65504.0; x[:, 2] = -65504.0; x[1, 3] = np.float16(6e-8); x[2, 3] = np.float16(-6e-8)      # +0, the range ends, subnormals
    state = (rng.choice(np.array([0, 1, 7], np.uint32), (3, V)) | np.where(rng.random((3, V)) < 0.5, PROMPT_BIT, np.uint32(0))).astype(np.uint32)
    bias = np.zeros((3, V), np.float32)
    p = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (3, 1))
    out = W.logit_adjust_rows(_dev(x), _dev(np.array([2, 0, 1], np.int32)), _dev(state.view(np.int32)), _dev(bias), _dev(p)).cpu().numpy()
    assert np.array_equal(out.view(np.uint16), x.view(np.uint16))
    # the one finite value the identity cannot hold for under the five steps as written: -0 + (+0 bias) = +0 (the numpy restatement agrees)
    z = np.full((1, V), -0.0, np.float16)
    outz = W.logit_adjust_rows(_dev(z), _dev(np.zeros(1, np.int32)), _dev(state.view(np.int32)), _dev(bias), _dev(p)).cpu().numpy()
    assert np.array_equal(outz.view(np.uint16)[0], restate(z[0], state[0], bias[0], p[0])) and not outz.view(np.uint16).any()


def test_state_kernels_against_a_histogram():
    V, slots = 1003, 4
    rng = np.random.default_rng(11)
    state = _dev(rng.integers(0, 2 ** 31, (slots, V)).astype(np.int32))          # garbage that a reset must clear
    bias = _dev(rng.normal(0, 1, (slots, V)).astype(np.float32))
    params = _dev(np.full((slots, 3), 9.0, np.float32))
    before = (state.cpu().numpy().copy(), bias.cpu().numpy().copy(), params.cpu().numpy().copy())
    prompt = np.array([5, 9, 5, 5, 1002, 0, 9, 77], np.int32)                     # duplicates
    bids, bvals = np.array([3, 1002, 40], np.int32), np.array([5.0, -np.inf, -100.0], np.float32)
    W.logit_state_reset(2, _dev(prompt), 1.3, 0.5, -0.25, _dev(bids), _dev(bvals), state, bias, params)
    want = np.zeros(V, np.uint32)
    want[prompt] |= PROMPT_BIT
    launches = [([2, 2, 2, 2], [5, 5, 7, 1002]), ([2, 2, 2], [7, 7, 7]), ([2, 2, 2, 2, 2], [0, 5, 600, 600, 7])]
    for sl, tk in launches:                                                       # repeated (slot, token) pairs
        W.logit_state_add(_dev(np.array(sl, np.int32)), _dev(np.array(tk, np.int32)), state)
        np.add.at(want, np.array(tk), np.uint32(1))
    torch.cuda.synchronize()
    st = state.cpu().numpy().view(np.uint32)
    assert np.array_equal(st[2], want)
    assert st[2, 5] == (PROMPT_BIT | np.uint32(3)) and st[2, 7] == 5 and st[2, 600] == 2 and st[2, 9] == PROMPT_BIT
    wb = np.zeros(V, np.float32); wb[bids] = bvals
    assert np.array_equal(bias.cpu().numpy()[2], wb)
    assert np.array_equal(params.cpu().numpy()[2], np.array([1.3, 0.5, -0.25], np.float32))
    for s in (0, 1, 3):                                                           # the other slots are nobody's business
        assert np.array_equal(st[s], before[0].view(np.uint32)[s]) and np.array_equal(bias.cpu().numpy()[s], before[1][s])
        assert np.array_equal(params.cpu().numpy()[s], before[2][s])
    # pairs outside the arrays are skipped, not written
    W.logit_state_add(_dev(np.array([4, -1, 2, 2], np.int32)), _dev(np.array([5, 5, V, -1], np.int32)), state)
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy().view(np.uint32)[2], want)
    # a second reset clears everything
    W.logit_state_reset(2, None, 1.0, 0.0, 0.0, None, None, state, bias, params)
    torch.cuda.synchronize()
    assert not state.cpu().numpy()[2].any() and not bias.cpu().numpy()[2].any()
    assert np.array_equal(params.cpu().numpy()[2], np.array([1.0, 0.0, 0.0], np.float32))
