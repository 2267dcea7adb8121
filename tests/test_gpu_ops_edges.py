"""-m gpu: every launch of csrc/ifa_ops.hip that a prompt step or a batched step runs between its GEMMs and its attention, against
float64 and the oracle at the edges of its launch geometry (cases, bounds, checks: tests/ops_edges_util.py; the host-side proof that
the checks reject the designed faults: tests/test_ops_edges_ref_cpu.py; branch map and recorded figures: docs/prompt_ops_edges.md).
The device-math constants are the host-measured ones doubled (ops_edges_util.dev_consts); none comes from a device result."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
import oracle as o
from tests import gpu_util as g
from tests import ops_edges_util as U

pytestmark = pytest.mark.gpu
K = U.dev_consts()
ERR_STATE = -4


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _slot(t, i):
    """the address of word i of an int32 tensor"""
    return C.c_void_p(t.data_ptr() + 4 * i)


def _off(a, pad=1):
    """the array on the device, starting `pad` elements into a larger buffer: 2 * pad bytes off 16-byte alignment"""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + 16, dtype=torch.float16, device="cuda")
    view = buf[pad:pad + a.size]
    view.copy_(g.dev(a).reshape(-1))
    assert view.data_ptr() % 16 == (2 * pad) % 16
    return view


# ------------------------------------------------------------------ RoPE
def _rope(c, x=None):
    xd = g.dev(c.x if x is None else x)
    if c.table:
        ia.check(g.capi().ifa_rope_rows(g.p(xd), c.hd, c.heads, c.tokens, g.p(_i32(c.pos)), c.theta, c.order, c.partial, g.stream()))
    else:
        ia.check(g.capi().ifa_rope(g.p(xd), c.hd, c.heads, c.tokens, int(c.pos0), c.theta, c.order, c.partial, g.stream()))
    return g.host(xd)


ROPE = U.rope_cases()


@pytest.mark.parametrize("c", ROPE, ids=[c.id for c in ROPE])
def test_rope(c):
    got = _rope(c)
    U.note("ifa_rope", U.check_rope(got, c, K["rope"]))
    if c.id.startswith("hd128-h4-t3-p57"):          # the stated bound of tests/test_gpu_ops.py::test_rope holds on its shape
        assert np.abs(got.astype(np.float32) - c.oracle().astype(np.float32)).max() <= 4e-3


ROWS = U.rope_rows_cases()


@pytest.mark.parametrize("c", ROWS, ids=[c.id for c in ROWS])
def test_rope_rows(c):
    got = _rope(c)
    U.note("ifa_rope_rows", U.check_rope(got, c, K["rope"], "rope_rows"))
    for t in range(c.tokens):                       # bit-identical to one ifa_rope call per row at that row's position
        xd = g.dev(c.x[t:t + 1])
        ia.check(g.capi().ifa_rope(g.p(xd), c.hd, c.heads, 1, int(c.pos[t]), c.theta, c.order, c.partial, g.stream()))
        assert U.same_bits(g.host(xd)[0], got[t]), (c.id, t)


def _store(c, q_view=None):
    L = g.capi()
    q, k, v = g.dev(c.q.x), g.dev(c.k.x), g.dev(c.v)
    kc = vc = None
    kp = vp = None
    if c.caches:
        kc, vc = g.dev(c.sentinel_cache()), g.dev(c.sentinel_cache())
        kp, vp = kc.data_ptr() + 2 * c.pos0 * c.row_elems, vc.data_ptr() + 2 * c.pos0 * c.row_elems
    rc = L.ifa_rope_qk_store(g.p(q), g.p(k), g.p(v), c.hd, c.heads, c.kv_heads, c.tokens, c.pos0, c.theta, c.order, c.partial, kp, vp, c.row_elems, g.stream())
    return rc, g.host(q), g.host(k), g.host(v), (g.host(kc).view(np.uint16) if c.caches else None), (g.host(vc).view(np.uint16) if c.caches else None)


STORE = U.store_cases() + [U.StoreCase(128, 254, 254, tokens=1, pos0=2, seed=20)]      # the last: 64 KiB of LDS, the largest accepted


@pytest.mark.parametrize("c", STORE, ids=[c.id for c in STORE])
def test_rope_qk_store(c):
    rc, q, k, v, kc, vc = _store(c)
    assert rc == 0, (c.id, rc, g.capi().ifa_last_error())
    U.note("ifa_rope_qk_store (%s path)" % ("vector" if c.vector else "scalar"), U.check_store(c, q, k, v, kc, vc, K["rope"], _rope(c.q), _rope(c.k)))


def test_rope_qk_store_refusals_next_to_accepted_calls():
    """every refusal returns IFA_ERR_STATE before any launch; the call each was made from is accepted (test_rope_qk_store runs the
    shapes: hd64-h4-kv4 and the 64 KiB case).  The table's addresses are replaced by real buffers that hold the largest shape of
    the table, so a wrapper that forgot a check would fail the assertion, not read unmapped memory; "vcache without v" has a null
    v by nature and stays with the host-only table (tests/test_ops_edges_ref_cpu.py, machines without a device)."""
    L = g.capi()
    base, refusals = U.store_refusals()
    need = max(a["tokens"] * max(a["heads"] * a["hd"], a["kv_heads"] * a["hd"], a["row_elems"]) for _, a in refusals) + 64
    real = {n: torch.zeros(need, dtype=torch.float16, device="cuda") for n in ("q", "k", "v", "kc", "vc")}
    ran = 0
    for why, a in refusals:
        if not a["v"]:
            continue
        ptr = {n: C.c_void_p(real[n].data_ptr() + a[n] - base[n]) for n in real}
        rc = L.ifa_rope_qk_store(ptr["q"], ptr["k"], ptr["v"], a["hd"], a["heads"], a["kv_heads"], a["tokens"], a["pos0"], a["theta"], a["order"], a["partial"],
                                 ptr["kc"], ptr["vc"], a["row_elems"], g.stream())
        assert rc == ERR_STATE, (why, rc)
        ran += 1
    assert ran == 11
    g.sync()
    assert all(float(t.abs().max()) == 0.0 for t in real.values())          # and nothing was written
    c = U.StoreCase(64, 4, 2, tokens=2, pos0=0, caches=False, seed=3)
    rc, q, k, v, _, _ = _store(c)
    assert rc == 0
    U.check_store(c, q, k, v, None, None, K["rope"])
    # a q that starts one element into its buffer: refused, q untouched -- never launched with it
    qv, k2, v2 = _off(c.q.x), g.dev(c.k.x), g.dev(c.v)
    rc = L.ifa_rope_qk_store(g.p(qv), g.p(k2), g.p(v2), c.hd, c.heads, c.kv_heads, c.tokens, c.pos0, c.theta, c.order, c.partial, None, None, c.row_elems, g.stream())
    assert rc == ERR_STATE
    g.sync()
    assert U.same_bits(g.host(qv), c.q.x.reshape(-1)) and U.same_bits(g.host(k2), c.k.x)


# ------------------------------------------------------------------ norms
def _norm(kind, x, w, b, mb, y=None, eps=1e-5):
    rows, cols = x.shape
    xd = x if torch.is_tensor(x) else g.dev(x)
    y = g.empty_f16(rows, cols) if y is None else y
    wd = w if (w is None or torch.is_tensor(w)) else g.dev(w)
    bd = b if (b is None or torch.is_tensor(b)) else g.dev(b)
    ia.check(g.capi().ifa_layernorm(kind, g.p(xd), rows, cols, g.p(wd), g.p(bd), mb, eps, g.p(y), g.stream()))
    return g.host(y).reshape(rows, cols)


@pytest.mark.parametrize("kind", [0, 1], ids=["rms", "std"])
@pytest.mark.parametrize("cols", U.NORM_COLS)
def test_layernorm(kind, cols):
    xa, xb, w, b = U.norm_inputs(cols, 3)
    name = "ifa_layernorm kind %d (%s)" % (kind, "16-byte paths" if cols % 8 == 0 else "ragged paths")
    for x in (xa, xb, xa[:1], xb[:1]):
        for form in U.NORM_FORMS:
            wv, bv, mb = U.form_args(form, w, b)
            if kind == 1 and form == "w+1":
                continue
            U.note(name, U.check_norm(kind, _norm(kind, x, wv, bv, mb), x, wv, bv, mb, "%s cols %d %s" % (name, cols, form)))


@pytest.mark.parametrize("kind", [0, 1], ids=["rms", "std"])
@pytest.mark.parametrize("cols", U.NORM_COLS)
def test_add_layernorm_and_the_engine_aliasing(kind, cols):
    """sum_out bit-exact with o.add, y bit-identical to ifa_layernorm of that sum_out; out of place, and in the two forms
    layer_forward uses: sum_out == addend (Add(x, attn out) + ffn norm) and sum_out == a (Add(ffn out, residual) + next norm)"""
    L = g.capi()
    xa, xb, w, b = U.norm_inputs(cols, 3)
    for rows in (3, 1):
        a, addend = xa[:rows], xb[:rows].copy()
        addend[0] = np.float16(0.3) * xb[1]
        for form in U.NORM_FORMS:
            wv, bv, mb = U.form_args(form, w, b)
            if kind == 1 and form == "w+1":
                continue
            for alias in ("none", "addend", "a"):
                ad, dd = g.dev(a), g.dev(addend)
                sd = {"none": g.empty_f16(rows, cols), "addend": dd, "a": ad}[alias]
                y = g.empty_f16(rows, cols)
                ia.check(L.ifa_add_layernorm(kind, g.p(ad), g.p(dd), rows, cols, g.p(g.dev(wv)) if wv is not None else None, g.p(g.dev(bv)) if bv is not None else None,
                                             mb, 1e-5, g.p(sd), g.p(y), g.stream()))
                s, yh = g.host(sd), g.host(y)
                what = "ifa_add_layernorm kind %d cols %d %s alias %s" % (kind, cols, form, alias)
                U.note("ifa_add_layernorm kind %d" % kind, U.check_add_norm(kind, s, yh, a, addend, wv, bv, mb, what))
                assert U.same_bits(yh, _norm(kind, s, wv, bv, mb)), what + ": y is not ifa_layernorm(sum_out)"


def test_norm_lds_limit():
    """32768 columns: the largest row the staging forms hold (64 KiB of LDS); 32769 is refused with a message, nothing launched"""
    L = g.capi()
    cols = 32768
    xa, xb, w, b = U.norm_inputs(cols, 1)
    U.check_norm(1, _norm(1, xb, w, b, 0.0), xb, w, b, 0.0, "std 32768")
    U.check_norm(0, _norm(0, xb, w, b, 0.0), xb, w, b, 0.0, "rms 32768")
    for kind in (0, 1):
        sd, y = g.empty_f16(1, cols), g.empty_f16(1, cols)
        ia.check(L.ifa_add_layernorm(kind, g.p(g.dev(xa)), g.p(g.dev(xb)), 1, cols, g.p(g.dev(w)), None, 0.0, 1e-5, g.p(sd), g.p(y), g.stream()))
        U.check_add_norm(kind, g.host(sd), g.host(y), xa, xb, w, None, 0.0, "add_layernorm 32768 kind %d" % kind)
    x = g.empty_f16(1, 32776)
    assert L.ifa_layernorm(1, g.p(x), 1, 32769, None, None, 0.0, 1e-5, g.p(x), g.stream()) == -1 and b"32768" in L.ifa_last_error()
    assert L.ifa_add_layernorm(0, g.p(x), g.p(x), 1, 32769, None, None, 0.0, 1e-5, g.p(x), g.p(x), g.stream()) == -1 and b"32768" in L.ifa_last_error()


@pytest.mark.parametrize("kind", [0, 1], ids=["rms", "std"])
@pytest.mark.parametrize("cols", [8, 512, 520])
def test_norm_pointer_alignment(kind, cols):
    """cols % 8 == 0 with a base that is not 16-byte aligned: k_layernorm takes its element-wise paths, which round the same
    expressions -- the same bits as the aligned launch, whichever operand is the one off alignment"""
    L = g.capi()
    xa, xb, w, b = U.norm_inputs(cols, 3)
    want = _norm(kind, xb, w, b, 0.0)
    U.check_norm(kind, want, xb, w, b, 0.0, "aligned")
    for which in ("x", "y", "w", "b"):
        xd = _off(xb).view(3, cols) if which == "x" else g.dev(xb)
        wd = _off(w) if which == "w" else g.dev(w)
        bd = _off(b, 3) if which == "b" else g.dev(b)
        ybuf = torch.zeros(3 * cols + 16, dtype=torch.float16, device="cuda")
        y = ybuf[1:1 + 3 * cols] if which == "y" else ybuf[:3 * cols]
        got = _norm(kind, xd, wd, bd, 0.0, y=y)
        assert U.same_bits(got, want), (kind, cols, which)
        assert (g.host(ybuf)[3 * cols + 1:] == 0).all() and (which != "y" or g.host(ybuf)[0] == 0)
    ad, dd, sbuf, y = g.dev(xa), _off(xb).view(3, cols), torch.zeros(3 * cols + 16, dtype=torch.float16, device="cuda"), g.empty_f16(3, cols)
    ia.check(L.ifa_add_layernorm(kind, g.p(ad), g.p(dd), 3, cols, g.p(g.dev(w)), g.p(g.dev(b)), 0.0, 1e-5, g.p(sbuf[1:]), g.p(y), g.stream()))
    U.check_add_norm(kind, g.host(sbuf)[1:1 + 3 * cols].reshape(3, cols), g.host(y), xa, xb, w, b, 0.0, "add_layernorm off alignment")
    assert g.host(sbuf)[0] == 0 and (g.host(sbuf)[3 * cols + 1:] == 0).all()


def test_norm_and_other_refusals_with_real_buffers():
    """the refusal tables of tests/test_ops_edges_ref_cpu.py (which hands out invented addresses, so only without a device) on
    buffers that hold the refused shape: a wrapper that forgot a check fails the assertion and reads mapped memory"""
    L = g.capi()
    x, i4 = g.empty_f16(1, 65552), _i32(np.zeros(8))
    err = L.ifa_last_error
    assert L.ifa_layernorm(1, g.p(x), 1, 65536, None, None, 0.0, 1e-5, g.p(x), g.stream()) == -1 and b"32768" in err()
    assert L.ifa_layernorm(0, g.p(x), 1, 65537, None, None, 0.0, 1e-5, g.p(x), g.stream()) == -1 and b"65536" in err()
    assert L.ifa_layernorm(2, g.p(x), 1, 8, None, None, 0.0, 1e-5, g.p(x), g.stream()) == -1 and b"kind" in err()
    assert L.ifa_layernorm(0, g.p(x), 1, 8, None, g.p(x), 0.0, 1e-5, g.p(x), g.stream()) == -1 and b"bias without weight" in err()
    assert L.ifa_add_layernorm(1, g.p(x), g.p(x), 1, 32769, None, None, 0.0, 1e-5, g.p(x), g.p(x), g.stream()) == -1 and b"32768" in err()
    assert L.ifa_layernorm(1, g.p(x), 0, 99999, None, None, 0.0, 1e-5, g.p(x), g.stream()) == 0          # no rows: nothing to do
    assert L.ifa_rope(g.p(x), 63, 1, 1, 0, 1e4, 2, 1.0, g.stream()) == -1 and b"head_dim" in err()
    assert L.ifa_rope(g.p(x), 64, 1, 1, 0, 1e4, 0, 1.0, g.stream()) == -1 and b"order" in err()
    assert L.ifa_rope_rows(g.p(x), 64, 1, 1, g.p(i4), 1e4, 3, 1.0, g.stream()) == -1 and b"order" in err()
    assert L.ifa_activation_mul(3, g.p(x), g.p(x), 8, g.p(x), g.stream()) == -1 and b"kind" in err()
    assert L.ifa_activation(-1, 0, g.p(x), 1, 8, g.p(x), g.stream()) == -1 and b"kind" in err()
    assert L.ifa_argmax(g.p(x), 0, g.p(i4), g.stream()) == -1 and L.ifa_argmax_masked(g.p(x), 0, None, g.p(i4), g.stream()) == -1
    assert L.ifa_argmax_rows(g.p(x), 0, 8, 1, g.p(i4), None, g.stream()) == -1 and L.ifa_argmax_rows(g.p(x), 8, 8, 0, g.p(i4), None, g.stream()) == 0


# ------------------------------------------------------------------ activation
def _act(kind, glu, x, rows, cols):
    y = g.empty_f16(rows, cols)
    ia.check(g.capi().ifa_activation(kind, glu, g.p(g.dev(x)), rows, cols, g.p(y), g.stream()))
    return g.host(y)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["silu", "gelu", "relu"])
def test_activation_over_every_finite_half(kind):
    v = U.all_finite_halves()
    got = _act(kind, 0, v, 1, v.size).reshape(-1)
    U.note("ifa_activation kind %d" % kind, U.check_act(got, v, kind, K, "ifa_activation kind %d" % kind))
    inf = np.array([np.inf, -np.inf] * 4, np.float16)
    gi, oi = _act(kind, 0, inf, 1, 8).reshape(-1), o.act(inf.reshape(1, -1), kind).reshape(-1)
    assert np.array_equal(np.isnan(gi), np.isnan(oi)) and np.array_equal(gi[~np.isnan(oi)], oi[~np.isnan(oi)])
    for cols in (1, 8, 100):
        x = np.random.default_rng(cols).normal(0, 2.0, (3, 2 * cols)).astype(np.float16)
        ref, tol = U.glu_f64(x, kind, K)
        U.note("ifa_activation glu", U.within(_act(kind, 1, x, 3, cols), ref, tol, "glu kind %d cols %d" % (kind, cols)))


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["silu", "gelu", "relu"])
def test_activation_mul(kind):
    L = g.capi()
    for n in U.ACT_MUL_N + [2048 + 1000]:
        a, b = U.act_mul_inputs(n)
        dev_act = _act(kind, 0, a, 1, n).reshape(-1)
        forms = [("out of place", g.dev(a), g.dev(b), None), ("in place", g.dev(a), g.dev(b), "a")]
        if n == 3048:           # n % 8 == 0 with one operand one element into its buffer: the two-launch fallback
            forms = [("a off alignment", _off(a), g.dev(b), None), ("b off alignment, in place", g.dev(a), _off(b), "a")]
        for name, ad, bd, alias in forms:
            cd = ad if alias else g.empty_f16(n)
            ia.check(L.ifa_activation_mul(kind, g.p(ad), g.p(bd), n, g.p(cd), g.stream()))
            path = "vector" if (n % 8 == 0 and n != 3048) else "fallback"
            U.note("ifa_activation_mul (%s)" % path, U.check_act_mul(g.host(cd), a, b, kind, K, "act_mul kind %d n %d %s" % (kind, n, name), dev_act))


# ------------------------------------------------------------------ argmax
@pytest.mark.parametrize("n", U.ARGMAX_N)
def test_argmax(n):
    """every vector of the length through the 16-byte scan and, one element into its buffer, through the scalar scan"""
    L = g.capi()
    vecs = U.argmax_vectors(n)
    out = torch.full((2 * len(vecs) + 1,), -7, dtype=torch.int32, device="cuda")
    for i, (name, v, words) in enumerate(vecs):
        for j, vd in enumerate((g.dev(v), _off(v))):
            slot = _slot(out, 2 * i + j)
            if words is None:
                ia.check(L.ifa_argmax(g.p(vd), n, slot, g.stream()))
            else:
                ia.check(L.ifa_argmax_masked(g.p(vd), n, g.p(_i32(words)), slot, g.stream()))
    got = out.cpu().numpy()
    assert got[-1] == -7
    for i, (name, v, words) in enumerate(vecs):
        ref = U.argmax_ref(v, U.excluded_of(words))
        assert got[2 * i] == ref and got[2 * i + 1] == ref, (n, name, int(got[2 * i]), int(got[2 * i + 1]), ref)


@pytest.mark.parametrize("stride", [1027, 1032])
def test_argmax_rows(stride):
    """5 rows; an odd stride puts every other row off 16-byte alignment (scalar scan); one result slot per row, the words behind untouched"""
    L = g.capi()
    rows, n = 5, 1025
    rng = np.random.default_rng(stride)
    buf = np.minimum(rng.normal(0, 1.0, rows * stride), 3.0).astype(np.float16)
    m = buf.reshape(rows, stride)
    m[0, [5, 900]] = 5.0
    m[1, [1024, 3]] = 5.0
    m[2, 1024] = 5.0
    m[3, [77, 512]] = 5.0
    m[3, n:] = 9.0              # past the row's n: never read as a candidate
    m[4, :n] = -np.inf
    for words in (None, U.excl_words([3, 77, 1024])[0], U.excl_words([5], 5)[0]):
        out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        ia.check(L.ifa_argmax_rows(g.p(g.dev(buf)), n, stride, rows, g.p(out), g.p(_i32(words)) if words is not None else None, g.stream()))
        got = out.cpu().numpy()
        assert got[:rows].tolist() == [U.argmax_ref(m[r, :n], U.excluded_of(words)) for r in range(rows)], (stride, words)
        assert (got[rows:] == -7).all()
    # every id of a 3-element row excluded: e0, e1, e2 leave no candidate in any row, aligned or not -- every slot becomes 0
    out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    ia.check(L.ifa_argmax_rows(g.p(g.dev(buf)), 3, stride, rows, g.p(out), g.p(_i32(U.excl_words([2, 0, 1])[0])), g.stream()))
    got = out.cpu().numpy()
    assert got[:rows].tolist() == [0] * rows and (got[rows:] == -7).all()


# ------------------------------------------------------------------ ALiBi, softmax
ALIBI = U.alibi_cases()


@pytest.mark.parametrize("c", ALIBI, ids=[c.id for c in ALIBI])
def test_alibi(c):
    sd = g.dev(c.s)
    ia.check(g.capi().ifa_alibi(g.p(sd), c.ctx, c.qt, c.heads, c.base, c.total, g.stream()))
    U.note("ifa_alibi", U.within(g.host(sd), c.ref, c.tol(K), "ifa_alibi " + c.id))


SOFTMAX = U.softmax_cases()


@pytest.mark.parametrize("c", SOFTMAX, ids=[c.id for c in SOFTMAX])
def test_softmax(c):
    sd = g.dev(c.s)
    ia.check(g.capi().ifa_softmax(g.p(sd), c.cx, c.cy, c.cz, c.prefix, c.scale, g.stream()))
    U.note("ifa_softmax", U.check_softmax(g.host(sd), c, K))


# ------------------------------------------------------------------ the cheap ops
@pytest.mark.parametrize("n", [1, 255, 257])
def test_add_mul_scale_row_index_bit_exact(n):
    L = g.capi()
    rng = np.random.default_rng(n)
    a, b = rng.normal(0, 1.0, n).astype(np.float16), rng.normal(0, 1.0, n).astype(np.float16)
    c = g.empty_f16(n)
    ia.check(L.ifa_add(g.p(g.dev(a)), g.p(g.dev(b)), n, 0, g.p(c), g.stream()))
    assert U.same_bits(g.host(c), o.add(a, b))
    period = min(n, 7)           # 7 does not divide 256: the period wraps inside a block
    ia.check(L.ifa_add(g.p(g.dev(a)), g.p(g.dev(b[:period])), n, period, g.p(c), g.stream()))
    assert U.same_bits(g.host(c), o.add(a, b[:period], period))
    ia.check(L.ifa_mul(g.p(g.dev(a)), g.p(g.dev(b)), n, g.p(c), g.stream()))
    assert U.same_bits(g.host(c), o.mul(a, b))
    ia.check(L.ifa_scale(g.p(g.dev(a)), 0.37, n, g.p(c), g.stream()))
    assert U.same_bits(g.host(c), o.scale(a, 0.37))
    A, B = rng.normal(0, 1, (3, n)).astype(np.float16), rng.normal(0, 1, (4, n)).astype(np.float16)
    idx, w = np.array([3, 0, 2], np.int32), rng.uniform(0, 1, 3).astype(np.float16)
    Bd = g.dev(B)
    ia.check(L.ifa_add_by_row_index(g.p(Bd), g.p(g.dev(A)), 3, n, g.p(_i32(idx)), g.p(g.dev(w)), g.stream()))
    exp = B.copy()
    for r in range(3):
        exp[idx[r]] = (A[r].astype(np.float64) * float(w[r]) + B[idx[r]].astype(np.float64)).astype(np.float16)
    assert U.same_bits(g.host(Bd), exp)


def test_worst_ratios_report():
    """prints the worst err / bound per launch of this run (docs/prompt_ops_edges.md records them)"""
    for k in sorted(U.WORST):
        print("ops-edges worst err/bound  %-42s %.3f" % (k, U.WORST[k]))
    assert all(v <= 1.0 for v in U.WORST.values())
