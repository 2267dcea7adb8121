"""-m gpu: the draft-aware logit processors (csrc/ifa_logit_adjust.hip, ifa_logit_adjust_draft_rows), F16 output bit for bit: row r
of a draft step equals ifa_logit_adjust_rows on a copy of the state that received ifa_logit_state_add of draft[0..r), and equals the
float32 numpy restatement of the five steps with w' = w + #{j < r : draft[j] == id}.  The op writes no state."""
import numpy as np
import pytest

import torch

import inferflow_amd  # noqa: F401
from inferflow_amd import worker as W
from tests.logit_adjust_util import PROMPT_BIT, restate

pytestmark = pytest.mark.gpu

SLOTS, SLOT = 3, 1
PARAMS = np.array([[1.0, 0.0, 0.0], [1.3, 0.5, -0.25], [0.5, -0.7, 1.0]], np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(V, rows, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 8, (rows, V)).astype(np.float16)
    x[:, 0] = 65504.0
    x[:, 1] = np.nan
    state = (rng.choice(np.array([0, 1, 7], np.uint32), (SLOTS, V)) | np.where(rng.random((SLOTS, V)) < 0.4, PROMPT_BIT, np.uint32(0))).astype(np.uint32)
    bias = np.zeros((SLOTS, V), np.float32)
    pick = rng.random((SLOTS, V))
    bias[pick < 0.06] = 5.0
    bias[(pick >= 0.06) & (pick < 0.12)] = -np.inf
    # the ids the drafts are made of (distinct, spread over the row; the last id of the row among them)
    a, b, c, d, last = [int(v) for v in (np.array([3, 11, 17, 24, V - 1]) % V)][:5]
    state[SLOT, a] = 1                      # generated once: a draft id twice makes it 3
    state[SLOT, b] = 0                      # never seen: the repetition rule newly fires
    state[SLOT, c] = PROMPT_BIT             # prompt only: the count becomes 1, bit 31 stays
    state[SLOT, d] = 2
    bias[SLOT, [a, b, c]] = 0.0
    bias[SLOT, d] = -np.inf                # banned: stays -inf whatever the count
    x[:, [a, b, c, d]] = np.array([4.0, -3.0, 2.5, 7.0], np.float16)
    return x, state, bias, (a, b, c, d, last)


def _drafts(rows, ids):
    a, b, c, d, last = ids
    if rows == 2:
        return [[a], [b], [c], [d]]
    return [[a, a, b, c, d, last, b][:rows - 1]]


def _place(x, stride, offset):
    """the rows in a buffer [rows][stride] that starts `offset` halfs into its allocation (offset 3: every input row off a 16-byte boundary)"""
    rows, V = x.shape
    flat = torch.zeros(offset + rows * stride, dtype=torch.float16, device="cuda")
    view = flat[offset:].view(rows, stride)[:, :V]
    view.copy_(_dev(x))
    return view


def _check(V, stride, offset, rows, params):
    x, state, bias, ids = _inputs(V, rows, seed=V * 8 + rows)
    lg = _place(x, stride, offset)
    st_dev, bias_dev, par_dev, slot_dev = _dev(state.view(np.int32)), _dev(bias), _dev(params), _dev(np.array([SLOT], np.int32))
    for draft in _drafts(rows, ids):
        d_dev = _dev(np.array(draft, np.int32))
        got = W.logit_adjust_draft_rows(lg, slot_dev, d_dev, st_dev, bias_dev, par_dev)
        again = W.logit_adjust_draft_rows(lg, slot_dev, d_dev, st_dev, bias_dev, par_dev)
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(np.uint16)
        assert got.shape == (rows, V) and np.array_equal(got, again.cpu().numpy().view(np.uint16))
        assert np.array_equal(st_dev.cpu().numpy().view(np.uint32), state)           # the state bytes are unchanged
        for r in range(rows):
            # the numpy rule on w'
            w = state[SLOT].copy()
            np.add.at(w, np.array(draft[:r], np.int64), np.uint32(1))
            want = restate(x[r], w, bias[SLOT], params[SLOT])
            bad = np.nonzero(got[r] != want)[0]
            assert bad.size == 0, (draft, r, bad[:8], got[r][bad[:8]], want[bad[:8]])
            # the existing op on a state copy that counted draft[0..r)
            st2 = _dev(state.view(np.int32))
            if r:
                W.logit_state_add(_dev(np.full(r, SLOT, np.int32)), d_dev[:r].contiguous(), st2)
            ref = W.logit_adjust_rows(lg, slot_dev, st2, bias_dev, par_dev, row_idx=_dev(np.array([r], np.int32)))
            assert np.array_equal(ref.cpu().numpy().view(np.uint16)[0], got[r]), (draft, r)
    return x, state, bias, ids, got


# 31: one workgroup, row 0 on the 16-byte path with a tail of 7, every other row id by id; 2048: exactly one workgroup of vectors;
# 2049: two workgroups, the second one only the tail id; (2048, 2056, 3): every input row off a 16-byte boundary, id by id
@pytest.mark.parametrize("rows", [2, 8])
@pytest.mark.parametrize("V,stride,offset", [(31, 31, 0), (2048, 2048, 0), (2049, 2049, 0), (2048, 2056, 3)])
def test_draft_rows_bit_exact(V, stride, offset, rows):
    x, state, bias, (a, b, c, d, last), got = _check(V, stride, offset, rows, PARAMS)
    if rows == 8:
        # the designed ids, worked out by hand from the five steps with {rep, freq, pres} = {1.3, 0.5, -0.25}
        f32, out = np.float32, got.view(np.float16)
        assert out[0, a] == np.float16(f32(4.0) / f32(1.3) - (f32(0.5) * f32(1.0) + f32(-0.25)))      # row 0: the state as it is
        assert out[2, a] == np.float16(f32(4.0) / f32(1.3) - (f32(0.5) * f32(3.0) + f32(-0.25)))      # behind a, a: 1 + 2
        assert out[2, b] == np.float16(-3.0) and out[3, b] == np.float16(f32(-3.0) * f32(1.3) - (f32(0.5) + f32(-0.25)))      # newly fires
        assert out[3, c] == np.float16(f32(2.5) / f32(1.3))                                           # bit 31 only: no count yet
        assert out[4, c] == np.float16(f32(2.5) / f32(1.3) - (f32(0.5) + f32(-0.25)))                 # count 1, bit 31 kept
        assert np.all(np.isneginf(out[:, d]))                                                         # banned in every row


@pytest.mark.parametrize("V,stride,offset", [(2049, 2049, 0), (2048, 2056, 3)])
def test_neutral_parameters_reproduce_the_input_bits(V, stride, offset):
    neutral = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (SLOTS, 1))
    x, state, bias, ids, got = _check(V, stride, offset, 8, neutral)
    free = bias[SLOT] == 0
    assert np.array_equal(got[:, free], x.view(np.uint16)[:, free])


def test_arguments_are_checked():
    from inferflow_amd import _capi
    x = torch.zeros((9, 64), dtype=torch.float16, device="cuda")
    z = torch.zeros((1, 64), dtype=torch.int32, device="cuda")
    with pytest.raises(_capi.IfaError, match="rows 9 outside 1..8"):
        W.logit_adjust_draft_rows(x, z[0, :1], z[0, :8], z, z.float(), torch.ones((1, 3), device="cuda"))
    with pytest.raises(_capi.IfaError, match="2 rows without draft tokens"):
        W.logit_adjust_draft_rows(x[:2], z[0, :1], None, z, z.float(), torch.ones((1, 3), device="cuda"))
