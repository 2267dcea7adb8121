"""-m gpu: the context shift at the worker level (csrc/ifa_kv_shift.hip).  ifa_kv_shift_rows against the numpy model of
tests/kv_shift_util.py byte for byte -- F16 and Q8 rows, both rope orders, partial rotary, no RoPE, row sizes and offsets that are
no multiple of 16 bytes, disjoint and overlapping ranges; ifa_model_kv_shift writes only what it should, whichever slot is
selected, and composes; the shifted layer-0 K rows ARE the rows of the compacted prompt; a one-layer model decodes behind shifted
rows what it decodes behind a fresh prompt of the compacted tokens; bad arguments are error codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth, worker as W
from tests import gpu_util as g
from tests import kv_shift_util as ku
from tests.test_gpu_prompt_routes import _agree

pytestmark = pytest.mark.gpu

CTX, SLOTS = 320, 3
# (shape, cache type, overrides)
CASES = [("test_gqa", dt.F16, {}), ("test_gqa", dt.Q8_B32T2, {}), ("test_mha", dt.F16, {}), ("test_mha", dt.Q8_B32T2, {}),
         ("test_falcon", dt.F16, {}), ("test_falcon", dt.Q8_B32T2, {}), ("test_tiny", dt.F16, {}),
         ("test_gqa", dt.F16, dict(partial_rotary=0.5)), ("test_gqa", dt.Q8_B32T2, dict(partial_rotary=0.5)),
         ("test_gqa", dt.F16, dict(rope_order=0, use_alibi=1)), ("test_gqa", dt.Q8_B32T2, dict(rope_order=0, use_alibi=1))]
# (keep, discard, n): two rows; disjoint; overlapping with a ragged last piece; one row dropped; everything but one row dropped;
# odd offsets; to the last row of the cache
TRIPLES = [(0, 1, 2), (4, 18, 40), (4, 5, 40), (7, 1, 40), (0, 39, 40), (3, 16, 35), (4, 158, 320)]


def _case_id(c):
    return "%s-%s%s" % (c[0], "f16" if c[1] == dt.F16 else "q8", "".join("-%s=%s" % kv for kv in sorted(c[2].items())))


def _geometry(c):
    s = dict(synth.SHAPES[c[0]])
    order = c[2].get("rope_order", s.get("rope_order", 2))
    cols = int(s["head_dim"] * c[2].get("partial_rotary", 1.0) + 0.5)
    return s["kv_heads"], s["head_dim"], order, cols, ku.row_bytes(c[1], s["kv_heads"], s["head_dim"])


class Model:
    def __init__(self, case):
        shape, kvd, over = case
        self.case, self.kvd = case, kvd
        self.wk, _, self.s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=CTX, **over)
        self.wk.kv_slots(SLOTS)
        self.kvh, self.hd, self.order, self.cols, self.rb = _geometry(case)
        self.layers, self.V = self.s["layers"], self.s["vocab"]
        rng = np.random.default_rng(17)
        self.prompts = [rng.integers(3, self.V, n).astype(np.int32) for n in (CTX, 48, 48)]      # slot 0: every row of the cache
        for slot, toks in enumerate(self.prompts):
            self.wk.select_kv(slot)
            self.wk.forward(toks, 0)
        self.snap = [self.read_slot(slot) for slot in range(SLOTS)]       # [slot][layer] -> (K bytes, V bytes); never modified
        for k, v in self.snap[0]:
            assert k.size == v.size == CTX * self.rb and k[-self.rb:].any() and v[-self.rb:].any()

    def read_slot(self, slot):
        self.wk.select_kv(slot)
        return [(self.wk.read_buffer("kcache", l), self.wk.read_buffer("vcache", l)) for l in range(self.layers)]

    def write_slot(self, slot, bufs):
        self.wk.select_kv(slot)
        for l, (k, v) in enumerate(bufs):
            self.wk.write_buffer("kcache", k, l)
            self.wk.write_buffer("vcache", v, l)

    def restore(self):
        for slot in range(SLOTS):
            self.write_slot(slot, self.snap[slot])


_MODELS = {}


def _model(case):
    key = _case_id(case)
    if key not in _MODELS:
        _MODELS[key] = Model(case)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.wk.close()
    _MODELS.clear()


@pytest.fixture(params=CASES, ids=_case_id)
def model(request):
    return _model(request.param)


# the layer-0 comparison is stated for an F16 cache of a RoPE model
F16_ROPE = [c for c in CASES if c[1] == dt.F16 and c[2].get("rope_order", 2) != 0]


def test_the_cases_cover_offsets_that_are_no_multiple_of_16_bytes():
    assert _geometry(CASES[1])[4] == 136 and _geometry(CASES[5])[4] == 68 and _geometry(CASES[0])[4] == 256 and _geometry(CASES[4])[4] == 128
    assert any(k * _geometry(c)[4] % 16 != 0 for c in CASES for k, _, _ in TRIPLES), "every keep * row_bytes is a multiple of 16"
    assert any(d * _geometry(c)[4] % 16 != 0 for c in CASES for _, d, _ in TRIPLES), "every discard * row_bytes is a multiple of 16"
    # the access widths these models meet: source and destination offsets whose common alignment is 16, 8 and 4 bytes (2 bytes:
    # test_rows_of_34_bytes_take_the_two_byte_accesses)
    widths = set()
    for c in CASES:
        rb = _geometry(c)[4]
        for k, d, _ in TRIPLES:
            a = (k * rb) | ((k + d) * rb)
            widths.add(next(w for w in (16, 8, 4, 2, 1) if a % w == 0))
    assert widths >= {16, 8, 4}, widths
    assert any(n - k - d > d and (n - k - d) % d for k, d, n in TRIPLES), "no overlapping case with a ragged last piece"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "k%d-d%d-n%d" % t)
def test_rows_op_equals_the_numpy_model(model, triple):
    """ifa_kv_shift_rows on copies of a layer's buffers with a random unit-circle table: every byte of both buffers equals the
    model's -- the moved rows, and rows [0, keep) and everything from row n - discard on untouched"""
    m = model
    keep, discard, n = triple
    rng = np.random.default_rng(1000 * keep + 10 * discard + n)
    table = ku.unit_table(m.hd, rng)
    layer = m.layers - 1
    k0, v0 = m.snap[0][layer]
    want_k, want_v = ku.shift(k0, v0, ku.F16 if m.kvd == dt.F16 else ku.Q8, m.kvh, m.hd, m.order, m.cols, table, keep, discard, n)
    kd, vd, td = _dev(k0), _dev(v0), _dev(table)
    m.wk.kv_shift_rows(kd.data_ptr(), vd.data_ptr(), td.data_ptr(), keep, discard, n)
    m.wk.sync()
    got_k, got_v = g.host(kd), g.host(vd)
    a, e = keep * m.rb, (n - discard) * m.rb
    assert np.array_equal(got_v, want_v), ("V", int(np.flatnonzero(got_v != want_v)[0]) // m.rb)
    assert np.array_equal(got_k, want_k), ("K", int(np.flatnonzero(got_k != want_k)[0]) // m.rb)
    for got, old in ((got_k, k0), (got_v, v0)):          # (what the model's equality implies, said once more in the test's own words)
        assert np.array_equal(got[:a], old[:a]) and np.array_equal(got[e:], old[e:])
    if n - keep - discard > 0 and m.order != 0:
        assert not np.array_equal(got_k[a:e], k0[(keep + discard) * m.rb:n * m.rb]), "the K rows were not rotated"
    # one side skipped: the other side's buffer is not written
    kd2, vd2 = _dev(k0), _dev(v0)
    m.wk.kv_shift_rows(kd2.data_ptr(), None, td.data_ptr(), keep, discard, n)
    m.wk.sync()
    assert np.array_equal(g.host(kd2), want_k) and np.array_equal(g.host(vd2), v0)
    kd3, vd3 = _dev(k0), _dev(v0)
    m.wk.kv_shift_rows(None, vd3.data_ptr(), td.data_ptr(), keep, discard, n)
    m.wk.sync()
    assert np.array_equal(g.host(kd3), k0) and np.array_equal(g.host(vd3), want_v)


@pytest.mark.parametrize("order", [1, 2, 0])
def test_rows_of_34_bytes_take_the_two_byte_accesses(order):
    """one kv head of 32 with a Q8 cache: rows of 34 bytes, so an odd keep or discard leaves offsets that allow 2-byte accesses only.
    No model: the rows are quantised random halves."""
    rng = np.random.default_rng(34 + order)
    rows_n, hd = 41, 32
    k0 = ku.q8_quant(rng.normal(0, 1, (rows_n, 1, 1, 32)).astype(np.float16)).reshape(-1)
    v0 = ku.q8_quant(rng.normal(0, 1, (rows_n, 1, 1, 32)).astype(np.float16)).reshape(-1)
    assert k0.size == rows_n * 34
    table = ku.unit_table(hd, rng)
    td = _dev(table)
    for keep, discard, n in ((1, 2, 40), (3, 18, 40), (1, 5, 40), (0, 1, 2), (2, 2, 41)):
        assert ((keep * 34) | ((keep + discard) * 34)) % 4 != 0 or (keep, discard) == (2, 2)
        want_k, want_v = ku.shift(k0, v0, ku.Q8, 1, hd, order, hd, table, keep, discard, n)
        kd, vd = _dev(k0), _dev(v0)
        W.kv_shift_rows(dt.Q8_B32T2, kd.data_ptr(), vd.data_ptr(), 1, hd, order, hd, td.data_ptr(), keep, discard, n)
        torch.cuda.synchronize()
        assert np.array_equal(g.host(kd), want_k) and np.array_equal(g.host(vd), want_v), (keep, discard, n)


@pytest.mark.parametrize("k_off,v_off", [(2, 0), (4, 4), (8, 16), (0, 2), (16, 16)])
def test_buffers_that_do_not_start_an_allocation(k_off, v_off):
    """the one-layer op on pointers k_off / v_off bytes into an allocation: the access width follows the pointers' alignment too
    (rows of 256 bytes: the offsets alone would allow 16-byte vectors); an odd address is refused and moves nothing"""
    rng = np.random.default_rng(100 + k_off + v_off)
    kvh, hd, n, keep, discard = 2, 64, 40, 4, 18
    k0 = rng.normal(0, 1, n * kvh * hd).astype(np.float16).view(np.uint8)
    v0 = rng.normal(0, 1, n * kvh * hd).astype(np.float16).view(np.uint8)
    table = ku.unit_table(hd, rng)
    want_k, want_v = ku.shift(k0, v0, ku.F16, kvh, hd, 2, hd, table, keep, discard, n)
    pad = np.full(32, 0xA5, np.uint8)
    kd, vd, td = _dev(np.concatenate([pad[:k_off], k0, pad])), _dev(np.concatenate([pad[:v_off], v0, pad])), _dev(table)
    assert kd.data_ptr() % 16 == 0 and vd.data_ptr() % 16 == 0
    W.kv_shift_rows(dt.F16, kd.data_ptr() + k_off, vd.data_ptr() + v_off, kvh, hd, 2, hd, td.data_ptr(), keep, discard, n)
    torch.cuda.synchronize()
    assert np.array_equal(g.host(kd), np.concatenate([pad[:k_off], want_k, pad]))
    assert np.array_equal(g.host(vd), np.concatenate([pad[:v_off], want_v, pad]))
    rc = ia.lib().ifa_kv_shift_rows(dt.F16, C.c_void_p(kd.data_ptr() + k_off + 1), C.c_void_p(vd.data_ptr() + v_off), kvh, hd, 2, hd,
                                    C.c_void_p(td.data_ptr()), keep, discard, n, None)
    assert rc == -1 and b"aligned" in ia.lib().ifa_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(g.host(vd), np.concatenate([pad[:v_off], want_v, pad]))


@pytest.mark.parametrize("cur", [0, 1, 2], ids=["target-selected", "another-selected", "a-third-selected"])
def test_worker_call_writes_only_its_slot(model, cur):
    m = model
    m.restore()
    keep, discard, n = 4, 18, 40
    m.wk.select_kv(cur)
    m.wk.kv_shift(1, keep, discard, n)
    m.wk.sync()
    now = [m.read_slot(slot) for slot in range(SLOTS)]
    a, b, e = keep * m.rb, (keep + discard) * m.rb, n * m.rb
    for l in range(m.layers):
        for kv in (0, 1):
            for slot in (0, 2):
                assert np.array_equal(now[slot][l][kv], m.snap[slot][l][kv]), (slot, l, kv)
            got, old = now[1][l][kv], m.snap[1][l][kv]
            assert np.array_equal(got[:a], old[:a]) and np.array_equal(got[a + e - b:], old[a + e - b:]), (l, kv)
            if kv == 1 or m.order == 0:                   # V rows, and the K rows of a model without RoPE, move byte for byte
                assert np.array_equal(got[a:a + e - b], old[b:e]), (l, kv)
            else:
                assert not np.array_equal(got[a:a + e - b], old[b:e]), (l, "K rows not rotated")


def test_two_calls_back_to_back_compose(model):
    m = model
    first, second = (4, 5, 40), (2, 9, 35)                # (the first one overlaps: several launches; the second starts where it ended)
    m.restore()
    m.wk.kv_shift(0, *first)
    m.wk.sync()
    mid = m.read_slot(0)
    m.wk.kv_shift(0, *second)
    m.wk.sync()
    want = m.read_slot(0)
    m.restore()
    m.wk.kv_shift(0, *first)
    m.wk.kv_shift(0, *second)                             # no synchronisation in between: the stream orders them
    m.wk.sync()
    got = m.read_slot(0)
    for l in range(m.layers):
        for kv in (0, 1):
            assert np.array_equal(got[l][kv], want[l][kv]), (l, kv)
            assert not np.array_equal(mid[l][kv], want[l][kv])


def _fill(m, slot, toks, by_decode):
    m.wk.select_kv(slot)
    m.wk.reset()
    if not by_decode:
        m.wk.forward(toks, 0)
        return
    for i, t in enumerate(toks):
        m.wk.decode(int(t), i, 1, timed=False)


def _pair_bound(m, want_rows):
    """2^-9 * ||pair||_2 per element of K rows [rows][kv_heads][head_dim] (float64); 0 for the columns that are not rotated"""
    bound = np.zeros_like(want_rows)
    for _, i0, i1 in ku.pairs(m.hd, m.order, m.cols):
        norm = np.hypot(want_rows[..., i0], want_rows[..., i1])
        bound[..., i0] = bound[..., i1] = 2.0 ** -9 * norm
    return bound


@pytest.mark.parametrize("triple", [(4, 18, 40), (3, 16, 35)], ids=lambda t: "k%d-d%d-n%d" % t)
@pytest.mark.parametrize("case", F16_ROPE, ids=_case_id)
def test_shifted_layer0_rows_are_the_compacted_prompts_rows(case, triple):
    """layer-0 rows depend only on the token and its position: slot A holds X, slot B holds X[:keep] + X[keep + discard:] + filler
    (same length, same prompt route).  After the shift, A's K rows [keep, n - discard) are B's within 2^-9 * ||pair||_2 per
    element -- two F16 roundings and the fp32 angle error, the bound of tests/test_context_shift_cpu.py -- and farther than that
    before it."""
    m = _model(case)
    assert len(F16_ROPE) == 5
    keep, discard, n = triple
    rng = np.random.default_rng(3)
    X = rng.integers(3, m.V, n).astype(np.int32)
    Y = np.concatenate([X[:keep], X[keep + discard:], rng.integers(3, m.V, discard).astype(np.int32)])
    a, b, e = keep * m.rb, (keep + discard) * m.rb, n * m.rb
    for by_decode in (False, True):
        _fill(m, 0, X, by_decode)
        _fill(m, 1, Y, by_decode)
        A, B = m.read_slot(0)[0], m.read_slot(1)[0]
        clean = np.array_equal(B[1][a:a + e - b], A[1][b:e])
        if clean:
            break
    assert clean, "layer-0 V rows of the compacted prompt differ from the original's: the comparison is not clean"
    m.wk.kv_shift(0, keep, discard, n)
    m.wk.sync()
    A2 = m.read_slot(0)[0]
    rows = lambda buf, lo, hi: buf[lo:hi].view(np.float16).astype(np.float64).reshape(-1, m.kvh, m.hd)
    want, got, before = rows(B[0], a, a + e - b), rows(A2[0], a, a + e - b), rows(A[0], b, e)
    bound = _pair_bound(m, want)
    err = np.abs(got - want)
    print("max |error| / bound: %.3f" % float(np.max(err[bound > 0] / bound[bound > 0])))
    assert np.all(err <= bound), (int(np.argmax(err - bound)), float(np.max(err - bound)))
    assert np.any(np.abs(before - want) > bound), "the unshifted rows pass too: the test cannot fail"
    assert np.array_equal(A2[1][a:a + e - b], B[1][a:a + e - b])
    m.restore()


@pytest.mark.parametrize("kvd", [dt.F16, dt.Q8_B32T2], ids=["f16", "q8"])
def test_one_layer_model_decodes_behind_shifted_rows_like_behind_the_compacted_prompt(kvd):
    """with ONE layer every cache row depends only on its token and position, so the shift is exact up to its roundings: a decode step
    behind the shifted rows agrees with the same step behind a fresh prompt of the compacted tokens under the project's law
    between two prompt routes (tests/test_gpu_prompt_routes.py: cosine >= 0.9999, max |delta| <= 0.02 std + 0.01)"""
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=CTX, layers=1)
    try:
        wk.kv_slots(2)
        keep, discard, n = 4, 18, 40
        rng = np.random.default_rng(8)
        X = rng.integers(3, s["vocab"], n).astype(np.int32)
        tok = int(rng.integers(3, s["vocab"]))
        wk.select_kv(0)
        wk.forward(X, 0)
        wk.kv_shift(0, keep, discard, n)
        out0, _ = wk.decode(tok, n - discard, 1, timed=False)
        lg0 = wk.read_buffer("logits").view(np.float16).astype(np.float32)
        wk.select_kv(1)
        wk.forward(np.concatenate([X[:keep], X[keep + discard:]]), 0)
        out1, _ = wk.decode(tok, n - discard, 1, timed=False)
        lg1 = wk.read_buffer("logits").view(np.float16).astype(np.float32)
        ok, why = _agree(lg0, lg1)
        print("shifted vs compacted prompt: cos %.7f max|d| %.5f std %.4f" % why)
        assert ok, why
        # and the step does see the shift: behind the unshifted rows the logits are another row
        wk.select_kv(0)
        wk.reset()
        wk.forward(X, 0)
        wk.decode(tok, n, 1, timed=False)
        lg2 = wk.read_buffer("logits").view(np.float16).astype(np.float32)
        assert not np.array_equal(lg2, lg0)
    finally:
        wk.close()


def test_bad_arguments_are_error_codes(model):
    m = model
    m.restore()
    L, h = ia.lib(), m.wk._h
    for slot, keep, discard, n, word in ((0, 4, 0, 40, b"discard"), (0, 4, -1, 40, b"discard"), (0, 30, 11, 40, b"exceed"), (0, -1, 4, 40, b"keep"),
                                         (0, 4, 18, CTX + 1, b"max_ctx"), (SLOTS, 4, 18, 40, b"slot"), (-1, 4, 18, 40, b"slot")):
        assert L.ifa_model_kv_shift(h, slot, keep, discard, n) == -1, (slot, keep, discard, n)
        assert word in L.ifa_last_error(), (slot, keep, discard, n, L.ifa_last_error())
    raw = W.DecodeWorker(max_ctx=64, kv_dtype=dt.F16, **synth.SHAPES["test_gqa"])      # created, never finalized
    assert L.ifa_model_kv_shift(raw._h, 0, 4, 18, 40) == -1 and b"not finalized" in L.ifa_last_error()
    raw.close()
    with pytest.raises(ia.IfaError):
        m.wk.kv_shift(0, 4, 0, 40)
    assert L.ifa_model_kv_shift(h, 0, 22, 18, 40) == 0                # nothing behind the dropped rows: ok, nothing moves
    m.wk.sync()
    now = [m.read_slot(slot) for slot in range(SLOTS)]
    for slot in range(SLOTS):
        for l in range(m.layers):
            for kv in (0, 1):
                assert np.array_equal(now[slot][l][kv], m.snap[slot][l][kv]), (slot, l, kv)


def test_q8_cache_with_head_dim_48_is_refused():
    s = synth.SHAPES["test_tiny"]
    assert s["head_dim"] == 48
    buf = torch.zeros(64 * ku.row_bytes(ku.F16, s["kv_heads"], 48), dtype=torch.uint8, device="cuda")
    tab = torch.zeros(48, dtype=torch.float32, device="cuda")
    rc = ia.lib().ifa_kv_shift_rows(dt.Q8_B32T2, C.c_void_p(buf.data_ptr()), None, s["kv_heads"], 48, 2, 48, C.c_void_p(tab.data_ptr()), 4, 18, 40, None)
    assert rc == -1 and b"head_dim 48" in ia.lib().ifa_last_error()
    torch.cuda.synchronize()
    assert not g.host(buf).any()
