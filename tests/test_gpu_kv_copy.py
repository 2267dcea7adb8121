"""-m gpu: ifa_model_kv_copy at the worker level -- rows [0, n) of every layer's K and V from one query slot to another in one
launch.  Byte equality of the copied rows, not one byte written behind them (row sizes that are no multiple of the kernel's
16-byte pieces included), the other slots untouched, whichever slot is selected; a step behind copied rows is bit for bit the
step behind the original ones, and agrees with the uncached prompt within the project's bound between two prompt routes."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth, worker as W
from tests import gpu_util as g
from tests.test_gpu_prompt_routes import _agree

pytestmark = pytest.mark.gpu

CTX, SLOTS, P0, P12, SUFFIX = 320, 3, 40, 48, 7
CASES = [("test_gqa", dt.F16), ("test_gqa", dt.Q8_B32T2), ("test_mha", dt.F16), ("test_mha", dt.Q8_B32T2)]
NS = [1, 2, 7, 33, 40]


def _row_bytes(shape, kvd):
    s = synth.SHAPES[shape]
    return dt.row_bytes(kvd, s["kv_heads"] * s["head_dim"])


class Model:
    def __init__(self, shape, kvd):
        self.wk, _, self.s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=CTX)
        self.wk.kv_slots(SLOTS)
        self.rb = _row_bytes(shape, kvd)
        self.layers, self.V = self.s["layers"], self.s["vocab"]
        rng = np.random.default_rng(11)
        self.prompts = [rng.integers(3, self.V, n).astype(np.int32) for n in (P0, P12, P12)]
        self.suffix = rng.integers(3, self.V, SUFFIX).astype(np.int32)
        for slot, toks in enumerate(self.prompts):
            self.wk.select_kv(slot)
            self.wk.forward(toks, 0)
        self.snap = self.read_all()          # [slot][layer] -> (K bytes, V bytes), whole buffers; never modified
        for slot in range(SLOTS):
            for k, v in self.snap[slot]:
                assert k.size == v.size == CTX * self.rb and k.any() and v.any()

    def read_slot(self, slot):
        self.wk.select_kv(slot)
        return [(self.wk.read_buffer("kcache", l), self.wk.read_buffer("vcache", l)) for l in range(self.layers)]

    def read_all(self):
        return [self.read_slot(slot) for slot in range(SLOTS)]

    def restore(self):
        for slot in range(SLOTS):
            self.wk.select_kv(slot)
            for l, (k, v) in enumerate(self.snap[slot]):
                self.wk.write_buffer("kcache", k, l)
                self.wk.write_buffer("vcache", v, l)

    def logits_tap(self):
        return self.wk.read_buffer("logits").copy()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-%s" % (c[0], "f16" if c[1] == dt.F16 else "q8"))
def model(request):
    m = Model(*request.param)
    yield m
    m.wk.close()


def test_some_case_is_no_multiple_of_16_bytes():
    """the narrow tail of the kernel is exercised: a Q8_B32T2 row of kv_dim 128 is 4 * 34 = 136 bytes"""
    assert _row_bytes("test_gqa", dt.Q8_B32T2) == 136
    odd = [(c, n) for c in CASES for n in NS if n * _row_bytes(*c) % 16 != 0]
    assert odd, "every n * kv_row_bytes is a multiple of 16: the tail path is not covered"
    assert {n for _, n in odd} >= {1, 7, 33}


@pytest.mark.parametrize("n", NS)
def test_copy_is_exact_and_writes_nothing_behind_the_rows(model, n):
    m = model
    m.restore()
    m.wk.select_kv(2)                           # neither slot is the selected one
    m.wk.kv_copy(0, 1, n)
    m.wk.sync()
    now = m.read_all()
    cut = n * m.rb
    for l in range(m.layers):
        for kv in (0, 1):
            got, src, old = now[1][l][kv], m.snap[0][l][kv], m.snap[1][l][kv]
            assert np.array_equal(got[:cut], src[:cut]), (l, kv, "copied rows")
            assert np.array_equal(got[cut:], old[cut:]), (l, kv, "bytes behind the copied rows", int(np.flatnonzero(got[cut:] != old[cut:])[0]))
            for slot in (0, 2):
                assert np.array_equal(now[slot][l][kv], m.snap[slot][l][kv]), (slot, l, kv)


@pytest.mark.parametrize("cur", [0, 1, 2], ids=["source-selected", "destination-selected", "neither"])
def test_copy_resolves_the_selected_slot(model, cur):
    m = model
    m.restore()
    n = 33
    m.wk.select_kv(cur)
    m.wk.kv_copy(0, 1, n)
    m.wk.kv_copy(2, 0, 2)                       # a second call right behind the first, the other way round a slot
    m.wk.sync()
    now = m.read_all()
    for l in range(m.layers):
        for kv in (0, 1):
            a, b = n * m.rb, 2 * m.rb
            assert np.array_equal(now[1][l][kv][:a], m.snap[0][l][kv][:a]) and np.array_equal(now[1][l][kv][a:], m.snap[1][l][kv][a:])
            assert np.array_equal(now[0][l][kv][:b], m.snap[2][l][kv][:b]) and np.array_equal(now[0][l][kv][b:], m.snap[0][l][kv][b:])
            assert np.array_equal(now[2][l][kv], m.snap[2][l][kv])


def _suffix_step(m, slot, toks):
    """the step behind P0 cached rows of `slot`: (next token, logits rows as bits, the slot's buffers afterwards)"""
    m.wk.select_kv(slot)
    if len(toks) == 1:
        out, _ = m.wk.decode(int(toks[0]), P0, 1, timed=False)
        return int(out[0]), m.logits_tap(), m.read_slot(slot)
    lg = torch.empty((len(toks), m.V), dtype=torch.float16, device="cuda")
    tok = m.wk.forward(toks, P0, lg)
    return int(tok), g.host(lg).view(np.uint16).copy(), m.read_slot(slot)


@pytest.mark.parametrize("n_suffix", [SUFFIX, 1], ids=["forward-7", "decode-1"])
def test_step_behind_copied_rows_is_bit_identical(model, n_suffix):
    m = model
    m.restore()
    toks = m.suffix[:n_suffix]
    m.wk.kv_copy(0, 1, P0)
    tok1, lg1, kv1 = _suffix_step(m, 1, toks)
    tok0, lg0, kv0 = _suffix_step(m, 0, toks)
    assert tok1 == tok0
    assert np.array_equal(lg1, lg0)
    end = (P0 + n_suffix) * m.rb
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(kv1[l][kv][:end], kv0[l][kv][:end]), (l, kv)
            assert kv0[l][kv][P0 * m.rb:end].any()


def test_split_prompt_on_copied_rows_is_close_to_the_uncached_prompt(model):
    """last-row logits of 40 cached + 7 new tokens against ONE 47-token prompt on a zeroed slot: the law between two prompt routes
    (tests/test_gpu_prompt_routes.py: cosine >= 0.9999, max |delta| <= 0.02 std + 0.01)"""
    m = model
    m.restore()
    m.wk.kv_copy(0, 1, P0)
    _, lg1, _ = _suffix_step(m, 1, m.suffix)
    split = lg1.view(np.float16).astype(np.float32)[-1]
    m.wk.select_kv(2)
    m.wk.reset()
    lg = torch.empty((P0 + SUFFIX, m.V), dtype=torch.float16, device="cuda")
    m.wk.forward(np.concatenate([m.prompts[0], m.suffix]), 0, lg)
    whole = g.host(lg).astype(np.float32)[-1]
    ok, why = _agree(split, whole)
    print("split vs whole prompt: cos %.7f max|d| %.5f std %.4f" % why)
    assert ok, why


def test_bad_arguments_are_error_codes(model):
    m = model
    m.restore()
    L, h = ia.lib(), m.wk._h
    for src, dst, n, word in ((1, 1, 4, b"both slot"), (-1, 1, 4, b"source slot"), (SLOTS, 1, 4, b"source slot"), (0, SLOTS, 4, b"destination slot"),
                              (0, -1, 4, b"destination slot"), (0, 1, -1, b"rows"), (0, 1, CTX + 1, b"rows")):
        assert L.ifa_model_kv_copy(h, src, dst, n) == -1, (src, dst, n)
        assert word in L.ifa_last_error(), (src, dst, n, L.ifa_last_error())
    assert L.ifa_model_kv_copy(h, 0, 1, 0) == 0                     # nothing to copy: ok, no launch
    assert L.ifa_model_kv_copy(h, 0, 1, CTX) == 0                   # the whole cache is in range
    raw = W.DecodeWorker(max_ctx=64, kv_dtype=dt.F16, **synth.SHAPES["test_gqa"])      # created, never finalized
    assert L.ifa_model_kv_copy(raw._h, 0, 1, 1) == -1 and b"not finalized" in L.ifa_last_error()
    raw.close()
    with pytest.raises(ia.IfaError):
        m.wk.kv_copy(0, 0, 1)
    m.wk.sync()
    now = m.read_all()                                               # the refused calls moved nothing; the full copy moved slot 0
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(now[1][l][kv], m.snap[0][l][kv]) and np.array_equal(now[2][l][kv], m.snap[2][l][kv])
