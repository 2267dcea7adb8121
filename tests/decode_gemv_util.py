"""Reference, inputs and assertions of the decode-GEMV edge tests (tests/test_decode_gemv_ref_cpu.py on the host,
tests/test_gpu_decode_gemv_edges.py on the device).

One fused GEMV launch computes, per output row r,  y[r] = sum_b xs[b] * sum_{i in b} w[r, i] * code[i]  over the 32-value blocks b of the
quantised activation (int8 codes, one F16 scale xs per block) -- or sum_i w[r, i] * x[i] on F16 activations -- followed by its epilogue
(bias, scale, residual(s), activation, gate).  Three things live here:

  * the reference of one launch from the inputs the DEVICE had (Launch): per output element the oracle's F16 value in the reference's
    order (oracle.gemv_ax8 / gemv_f16x, then oracle.add / scale / act / mul as oracle.Model applies them) and the float64 value (the
    oracle's own fp64 sum through the same epilogue without any rounding);
  * input families (dense / sign / tail-only) and the block decomposition of the float64 product, on which the mutations are expressed:
    a block dropped, doubled or paired with another block's activation, the code-sum (zero-point) term omitted, the residual dropped
    or doubled, a row finished with its neighbour's sum;
  * the assertions the GPU test applies to a device output (check_exact, check_prologue), as functions, so that the CPU test can feed
    them MUTATED oracle outputs and see every one rejected.

Tolerances.  Exact-input launches (the activation image is known bit for bit): every element within max(2 x d_ref, one F16 ulp at
|out|) of float64, d_ref = max|oracle - float64| over the launch -- the criterion of docs/decode_attention_edges.md: the distance of the
reference's own rounding points from exact math, times 2 for another order of the fp32 sums.  Prologue launches (the device normalises
the input itself; its norm may differ from the oracle's in a last bit, which moves an F16 value by one ulp and with it, now and then, one
int8 code by one): a row may use, on top of that, F code flips of size max|w of the row| x max block scale of the activation
(flip_unit); at most FLIP_ROWS_MAX of a launch's rows may need the term at all.  F comes from a measurement on MI355X
(docs/decode_gemv_edges.md), never from the case under test.  A gated launch out = act(t1) x t3 carries the flips of both products:
F d1 x L x |t3| + |act(t1)| x F d3 + L x F d1 x F d3 with L = 1.13, the largest slope of SiLU (1.0998) and tanh-GELU (1.129)."""
import numpy as np

import oracle as o
from inferflow_amd import dtypes as dt
from tests.decode_attn_util import ulp16

SENSITIVITY = 5.0           # a mutation moves the float64 output by >= SENSITIVITY x bound in at least one row
FLIP_ROWS_MAX = 0.02        # share of a prologue launch's rows that may need the flip term
ACT_SLOPE = 1.13
EPI_PLAIN, EPI_RESIDUAL, EPI_GLU, EPI_ACT = 0, 1, 2, 3
Q3H_NATIVE = 99


def is_ax8(dtype):
    return dtype in dt.AX8


def capacity(dtype):
    return 8 if dtype == dt.F16 else dt.block_capacity(dtype)       # (F16: the 8-value chunk a lane loads)


def lane_round(dtype):
    """columns one round of the 64 lanes covers (F16 on the fp16-activation kernel: 4 chunks of 8 per lane and round)"""
    return 2048 if dtype == dt.F16 else 64 * dt.block_capacity(dtype)


def last_round_cols(dtype, cols):
    """the columns of the last round of blocks: the last cols mod L columns, or the last L when that is 0"""
    L = lane_round(dtype)
    n = cols % L or min(L, cols)
    return cols - n, cols


# ----------------------------------------------------------------------------- activations
def act_f64(v, kind):
    v = np.asarray(v, np.float64)
    if kind == 0:
        return v / (1.0 + np.exp(-v))
    if kind == 1:
        return 0.5 * v * (1.0 + np.tanh(0.79788456080286535587989211986876 * v * (1.0 + 0.044715 * v * v)))
    return np.maximum(v, 0.0)


def q8_image(x16):
    """F16 vector -> the reference quantiser's Q8_B32T2 row (34-byte blocks: F16 scale, 32 int8 codes)"""
    return o.quantize_act_q8(np.ascontiguousarray(x16, np.float16).reshape(1, -1))[0]


def q8_parts(image, cols):
    """-> (codes int64 [blocks][32], scales float64 [blocks])"""
    b = np.ascontiguousarray(image, np.uint8).reshape(cols // 32, 34)
    return b[:, 2:].view(np.int8).astype(np.int64), b[:, :2].copy().view(np.float16).astype(np.float64).reshape(-1)


def xq_image_to_q8(image, cols):
    """the device's quantised image of the attention output (xq_image_carve: codes [cols] padded to 16 bytes, fp32 value of the F16 block
    scale [cols / 32], fp32 code sums [cols / 32]) -> the same activation as a Q8_B32T2 row; the scales must be F16 values and the sums
    the sums of the codes"""
    img = np.ascontiguousarray(image, np.uint8)
    nb, off = cols // 32, (cols + 15) // 16 * 16
    codes = img[:cols].reshape(nb, 32)
    scale = img[off:off + 4 * nb].copy().view(np.float32)
    xsum = img[off + 4 * nb:off + 8 * nb].copy().view(np.float32)
    s16 = scale.astype(np.float16)
    assert np.array_equal(s16.astype(np.float32), scale), "attq: a block scale is not an F16 value"
    assert np.array_equal(xsum, codes.view(np.int8).astype(np.int32).sum(axis=1).astype(np.float32)), "attq: a code sum differs from its codes"
    row = np.zeros((nb, 34), np.uint8)
    row[:, :2] = s16.view(np.uint8).reshape(nb, 2)
    row[:, 2:] = codes
    return row.reshape(-1)


# ----------------------------------------------------------------------------- weights
class Mat:
    """one weight matrix in the reference byte layout (uint8 [rows][row bytes]; F16: values) with its float64 view"""

    def __init__(self, dtype, data, rows, cols, bias=None):
        self.dtype, self.rows, self.cols = dtype, rows, cols
        self.bias = None if bias is None else np.ascontiguousarray(bias, np.float16).reshape(-1)
        if dtype == dt.F16:
            self.data = np.ascontiguousarray(data).view(np.float16).reshape(rows, cols)
        else:
            self.data = np.ascontiguousarray(data, np.uint8).reshape(rows, dt.row_bytes(dtype, cols))
        self._w64 = self._base = None

    @property
    def w64(self):
        """the weights [rows][cols] as float64: scale x code + base as the block decoder gives them in fp32 (int8-path formats); the
        HALF-rounded dequantised value the fp16-activation kernels multiply (the other block formats); the F16 values"""
        if self._w64 is None:
            if self.dtype == dt.F16:
                w = self.data
            else:
                w = o.dequantize(self.dtype, self.data, self.cols, out_f32=is_ax8(self.dtype))
            self._w64 = w.astype(np.float64)
        return self._w64

    def wmax(self):
        return np.abs(self.w64).max(axis=1)

    def base(self):
        """the zero-point (code 0) value of every weight block [rows][cols / capacity]: the intercept of w = scale x code + base, fitted
        from the block's codes and values (0 where a block's codes are all equal, and for Q8_B32T2, which has none)"""
        if self._base is None:
            cap = dt.block_capacity(self.dtype)
            q = o.unpack_codes(self.dtype, self.data, self.cols).astype(np.float64).reshape(self.rows, -1, cap)
            w = self.w64.reshape(self.rows, -1, cap)
            qm, wm = q.mean(axis=2, keepdims=True), w.mean(axis=2, keepdims=True)
            var = ((q - qm) ** 2).sum(axis=2)
            slope = np.where(var > 0, ((q - qm) * (w - wm)).sum(axis=2) / np.maximum(var, 1e-30), 0.0)
            self._base = np.where(var > 0, wm[:, :, 0] - slope * qm[:, :, 0], 0.0)
            if self.dtype == dt.Q8_B32T2:
                self._base[:] = 0.0
        return self._base


# ----------------------------------------------------------------------------- one product and its block decomposition
class Product:
    """y = W . x of one matrix on one activation: the oracle's F16 result (bias added in half, as the reference does) and the float64
    value.  xq: a Q8_B32T2 row (int8-path formats); x16: F16 values (fp16-activation formats)."""

    def __init__(self, mat, xq=None, x16=None):
        self.mat = mat
        m = mat
        if is_ax8(m.dtype):
            assert xq is not None
            self.xq = np.ascontiguousarray(xq, np.uint8)
            y16, y64 = o.gemv_ax8(m.dtype, m.data, m.rows, m.cols, self.xq, want_f64=True)
            if m.bias is not None:
                y16 = o.add(y16, m.bias)
                y64 = y64 + m.bias.astype(np.float64)
            codes, xs = q8_parts(self.xq, m.cols)
            self.x64 = (codes * xs[:, None]).reshape(-1)
            self.xs_max = float(xs.max())
        else:
            assert x16 is not None
            self.x16 = np.ascontiguousarray(x16, np.float16).reshape(-1)
            y16, y64 = o.gemv_f16x(m.dtype, m.data, m.rows, m.cols, self.x16, m.bias, want_f64=True)
            self.x64 = self.x16.astype(np.float64)
            self.xs_max = float(ulp16(np.abs(self.x64).max()))      # (no codes: what a last bit of the norm moves is one F16 ulp of a value)
        self.y16, self.y64 = y16, y64
        self._blocks = None

    def blocks(self):
        """float64 [rows][weight blocks]: the contribution of every weight block (fp16 activations: 8-value chunk) to y"""
        if self._blocks is None:
            cap = capacity(self.mat.dtype)
            self._blocks = (self.mat.w64 * self.x64[None, :]).reshape(self.mat.rows, -1, cap).sum(axis=2)
        return self._blocks

    def other_block(self, j):
        """the nearest block k != j whose activation differs from block j's (pairing a weight block with an identical activation is no
        fault); None if there is none"""
        cap = capacity(self.mat.dtype)
        xb = self.x64.reshape(-1, cap)
        for d in range(1, xb.shape[0]):
            for k in (j + d, j - d):
                if 0 <= k < xb.shape[0] and not np.array_equal(xb[k], xb[j]):
                    return k
        return None

    def mispaired(self, j, k):
        """float64 [rows]: weight block j times activation block k"""
        cap = capacity(self.mat.dtype)
        return self.mat.w64[:, j * cap:(j + 1) * cap] @ self.x64[k * cap:(k + 1) * cap]

    def zero_point_term(self):
        """float64 [rows]: sum over the activation blocks a of xs[a] x base[r, weight block of a] x (sum of the codes of a) -- the code-sum
        term of the int8 kernels; None where the format has none"""
        m = self.mat
        if not is_ax8(m.dtype) or m.dtype == dt.Q8_B32T2:
            return None
        codes, xs = q8_parts(self.xq, m.cols)
        per_a = xs * codes.sum(axis=1)                                             # [activation blocks]
        per_w = per_a.reshape(-1, dt.block_capacity(m.dtype) // 32).sum(axis=1)    # [weight blocks]
        return m.base() @ per_w

    def flip_unit(self):
        """what one int8 code of the activation, off by one, can move a row by: max|w of the row| x the largest block scale (fp16
        activations: x one F16 ulp at the largest value)"""
        return self.mat.wmax() * self.xs_max


# ----------------------------------------------------------------------------- one launch
class Launch:
    """the reference of one fused GEMV launch.  products: the Product(s) whose rows are concatenated (Wq | Wk | Wv) -- or, gated, the
    pair (W1, W3); epi: EPI_*; res / res2: F16 residual vectors; pre / post: the Scale factors (None: absent); act_kind.  exact: the
    activation image is the device's own bit for bit (else the prologue bound applies)."""

    def __init__(self, name, products, epi, exact, res=None, res2=None, pre=None, post=None, act_kind=0):
        self.name, self.products, self.epi, self.exact, self.act_kind = name, products, epi, exact, act_kind
        self.res = None if res is None else np.ascontiguousarray(res, np.float16).reshape(-1)
        self.res2 = None if res2 is None else np.ascontiguousarray(res2, np.float16).reshape(-1)
        self.pre, self.post = pre, post
        self.orc = self._finish16([p.y16 for p in products]).astype(np.float64)
        self.f64 = self.finish64([p.y64 for p in products])
        self.d_ref = float(np.abs(self.orc - self.f64).max())
        self.bound = np.maximum(2.0 * self.d_ref, ulp16(self.f64))
        self.rows = self.f64.size

    def _finish16(self, ys):
        if self.epi == EPI_GLU:
            return o.mul(o.act(ys[0].reshape(1, -1), self.act_kind)[0], ys[1])
        if self.epi == EPI_ACT:
            return o.act(ys[0].reshape(1, -1), self.act_kind)[0]
        y = np.concatenate(ys)
        if self.pre is not None:
            y = o.scale(y, self.pre)
        if self.epi == EPI_RESIDUAL:
            y = o.add(self.res, y)
            if self.res2 is not None:
                y = o.add(y, self.res2)
            if self.post is not None:
                y = o.scale(y, self.post)
        return y

    def finish64(self, ys, res_times=1.0):
        """the epilogue in float64 without rounding; res_times: how often the residual is added (the mutations: 0, 2)"""
        if self.epi == EPI_GLU:
            return act_f64(ys[0], self.act_kind) * ys[1]
        if self.epi == EPI_ACT:
            return act_f64(ys[0], self.act_kind)
        y = np.concatenate(ys)
        if self.pre is not None:
            y = y * float(np.float32(self.pre))
        if self.epi == EPI_RESIDUAL:
            y = y + res_times * self.res.astype(np.float64)
            if self.res2 is not None:
                y = y + self.res2.astype(np.float64)
            if self.post is not None:
                y = y * float(np.float32(self.post))
        return y

    def flip_extra(self, F):
        """what F code flips may add to every row's bound (0 for an exact launch)"""
        if self.exact or F == 0:
            return np.zeros(self.rows)
        if self.epi == EPI_GLU:
            d1, d3 = F * self.products[0].flip_unit(), F * self.products[1].flip_unit()
            a1, t3 = np.abs(act_f64(self.products[0].y64, self.act_kind)), np.abs(self.products[1].y64)
            return ACT_SLOPE * d1 * t3 + a1 * d3 + ACT_SLOPE * d1 * d3
        u = F * np.concatenate([p.flip_unit() for p in self.products])
        if self.epi == EPI_ACT:
            return ACT_SLOPE * u
        s = (abs(self.pre) if self.pre is not None else 1.0) * (abs(self.post) if self.post is not None else 1.0)
        return u * s

    # -- mutations: float64 outputs of a launch with one systematic fault (every row)
    def mutations(self, blocks):
        """yields (name, float64 output): for product 0 and every weight block j of `blocks` -- dropped, doubled, paired with the
        activation of the nearest block that holds another one --, the zero-point term omitted (formats that have one), the
        residual dropped / doubled, every row finished with the next row's sum"""
        ys = [p.y64 for p in self.products]
        for pi, p in enumerate(self.products):
            if pi > 0 and self.epi != EPI_GLU:
                break                                    # (Wq | Wk | Wv: three matrices of one kind; the gated pair: both sides)
            B = p.blocks()
            nb = B.shape[1]

            def with_y(y):
                z = list(ys)
                z[pi] = y
                return self.finish64(z)

            for j in blocks:
                if j >= nb:
                    continue
                yield ("drop block %d of product %d" % (j, pi), with_y(p.y64 - B[:, j]))
                yield ("double block %d of product %d" % (j, pi), with_y(p.y64 + B[:, j]))
                k = p.other_block(j)
                if k is not None:
                    yield ("block %d of product %d on the activation of block %d" % (j, pi, k), with_y(p.y64 - B[:, j] + p.mispaired(j, k)))
            z = p.zero_point_term()
            if z is not None:
                yield ("zero-point term of product %d omitted" % pi, with_y(p.y64 - z))
            if p.mat.rows > 1:
                yield ("rows of product %d finished with the next row's sum" % pi, with_y(np.roll(p.y64, -1)))
        if self.epi == EPI_RESIDUAL:
            yield ("residual dropped", self.finish64(ys, 0.0))
            yield ("residual doubled", self.finish64(ys, 2.0))


def probed_blocks(dtype, cols, sample=(0, 1, 63, 64, 65)):
    """the weight blocks whose loss a test must notice: every block of the last round and a sample of the others"""
    cap = capacity(dtype)
    lo, hi = last_round_cols(dtype, cols)
    nb = cols // cap
    return sorted(set(range(lo // cap, hi // cap)) | {j for j in sample if j < nb})


# ----------------------------------------------------------------------------- inputs
SEED_LONG = 3000            # the 256-value layer input of the long models


def seed_of(cols):
    """the seed of the layer input of a model whose QKV and W1 / W3 see `cols` columns (wide family, rows, wirings)"""
    return 1000 + cols


def make_input(family, cols, dtype, seed):
    """the F16 layer input of a case.  dense: N(0, 1).  sign: +-1 -- the RMS norm scales by 1 / sqrt(1 + eps), which rounds back to +-1 in
    F16 whatever the last bit of the scale, so the Q8 image is +-127 with one scale (1 / 127 in F16) and a prologue launch is exactly
    comparable.  tail: zero except the columns of the last round of blocks of a `dtype` row (N(0, 1) there)."""
    rng = np.random.default_rng(seed)
    if family == "dense":
        return rng.normal(0, 1, cols).astype(np.float16)
    if family == "sign":
        return np.where(rng.integers(0, 2, cols) == 0, -1.0, 1.0).astype(np.float16)
    if family == "tail":
        x = np.zeros(cols, np.float16)
        lo, hi = last_round_cols(dtype, cols)
        x[lo:hi] = rng.normal(0, 1, hi - lo).astype(np.float16)
        return x
    raise ValueError(family)


def std_norm_affine(cols):
    """weight and bias (F16) of the std-norm wiring's norms: 1 + N(0, 0.1) and N(0, 0.3).  A std norm with unit weights and no bias
    hands on a vector whose values add up to 0, and with it Q8 code sums that cancel over a row of one or two blocks: the zero-point
    term of the int8 kernels would vanish at the smallest widths and its loss could not be seen there"""
    rng = np.random.default_rng(7000 + cols)
    return (1.0 + rng.normal(0, 0.1, cols)).astype(np.float16), rng.normal(0, 0.3, cols).astype(np.float16)


def norm_exact(family, norm_kind, norm_w):
    """True if the normalised vector of this family is the same F16 values whatever the last bits of the norm's statistics: the sign
    family behind an RMS norm with unit weights"""
    return family == "sign" and norm_kind == 0 and norm_w is not None and bool(np.all(np.asarray(norm_w, np.float32) == 1.0))


def perturbed_norms(x16, eps=1e-5):
    """the RMS-normalised input (unit weights) with the fp32 scale one ulp down, as is, and one ulp up: F16 vectors.  What a device whose
    sum of squares differs in the last bit hands to its quantiser."""
    x = np.asarray(x16, np.float16).astype(np.float32)
    scale = np.float32(1.0) / np.sqrt(np.float32(np.mean(x.astype(np.float64) ** 2)) + np.float32(eps), dtype=np.float32)
    return [o.f2h(x * s) for s in (np.nextafter(scale, np.float32(0)), scale, np.nextafter(scale, np.float32(2) * scale))]


# ----------------------------------------------------------------------------- the assertions on a device output
def flips_needed(out16, launch, fmax=64):
    """per row: the smallest F >= 0 with |out - float64| <= bound + flip_extra(F) (fmax + 1: none up to fmax)"""
    err = np.abs(np.asarray(out16).astype(np.float64).reshape(-1) - launch.f64)
    need = np.full(launch.rows, fmax + 1, np.int64)
    for F in range(fmax, -1, -1):
        need[err <= launch.bound + launch.flip_extra(F)] = F
    return need


def violations(out16, launch, F=0):
    """rows of out16 beyond the launch's bound (the exact bound; a prologue launch: + F flips): what check() asserts to be 0"""
    a = np.asarray(out16).astype(np.float64).reshape(-1)
    return int((~(np.abs(a - launch.f64) <= launch.bound + launch.flip_extra(0 if launch.exact else F))).sum())


def check_exact(out16, launch):
    """out16: the launch's output under test.  Asserts every element within max(2 x d_ref, one F16 ulp at |out|) of float64; returns
    (median, worst) of err / bound"""
    a = np.asarray(out16).astype(np.float64).reshape(-1)
    assert a.size == launch.rows, (launch.name, a.size, launch.rows)
    assert np.isfinite(a).all(), "%s: output is not finite" % launch.name
    r = np.abs(a - launch.f64) / launch.bound
    w = int(r.argmax())
    assert r[w] <= 1.0, "%s: row %d is %.3g from float64, bound %.3g (d_ref %.3g; %d of %d rows over)" % (
        launch.name, w, abs(a[w] - launch.f64[w]), launch.bound[w], launch.d_ref, int((r > 1.0).sum()), r.size)
    return float(np.median(r)), float(r[w])


def check_prologue(out16, launch, F):
    """a launch behind the device's own norm: every row within the exact bound + F code flips, at most FLIP_ROWS_MAX of the rows
    beyond the exact bound.  Returns (median, worst err / exact bound, share of rows using the
    flip term, most flips a row needed)"""
    a = np.asarray(out16).astype(np.float64).reshape(-1)
    assert a.size == launch.rows, (launch.name, a.size, launch.rows)
    assert np.isfinite(a).all(), "%s: output is not finite" % launch.name
    err = np.abs(a - launch.f64)
    r = err / launch.bound
    over = err > launch.bound + launch.flip_extra(F)
    w = int((err - launch.bound - launch.flip_extra(F)).argmax())
    assert not over.any(), "%s: row %d is %.3g from float64, bound %.3g + %d flips %.3g (%d of %d rows over)" % (
        launch.name, w, err[w], launch.bound[w], F, launch.flip_extra(F)[w], int(over.sum()), r.size)
    share = float((r > 1.0).mean())
    assert share <= FLIP_ROWS_MAX, "%s: %.1f %% of the rows need the flip term (at most %.1f %%)" % (launch.name, 100 * share, 100 * FLIP_ROWS_MAX)
    need = flips_needed(out16, launch, F)
    return float(np.median(r)), float(r.max()), share, int(need.max())


def check(out16, launch, F):
    """the assertion of the launch's kind; returns (median, worst, share of rows on the flip term, most flips needed)"""
    if launch.exact:
        med, worst = check_exact(out16, launch)
        return med, worst, 0.0, 0
    return check_prologue(out16, launch, F)


# ----------------------------------------------------------------------------- the launches of one decode step of a one-layer model
class Model:
    """what the references of a step need of a one-layer model: cfg (dict: dim, heads, kv_heads, head_dim, ffn, norm_kind, act_kind,
    is_glu, parallel_attn, share_input, eps, attn_out_scale, ffn_out_scale, out_scale), mats (name -> Mat for wq wk wv wo w1 w3 w2, biases
    inside) and the norm vectors (attn_norm, attn_norm_b, ffn_norm, ffn_norm_b: F16 or None)"""

    def __init__(self, cfg, mats, norms):
        self.cfg, self.mats, self.norms = cfg, mats, norms


def _scale_on(s):
    return s is not None and (s < 0.9999 or s > 1.0001)          # (the engine's and the reference's test for "scale != 1")


def _norm(model, x16, which):
    c = model.cfg
    w, b = model.norms.get(which), model.norms.get(which + "_b")
    x = np.ascontiguousarray(x16, np.float16).reshape(1, -1)
    if c.get("norm_kind", 0) == 0:
        return o.rmsnorm(x, w, b, 0.0, c.get("eps", 1e-5))[0]
    return o.stdnorm(x, w, b, c.get("eps", 1e-5))[0]


def _product(mat, x16=None, xq=None):
    if is_ax8(mat.dtype):
        return Product(mat, xq=xq if xq is not None else q8_image(x16))
    assert x16 is not None, "an fp16-activation format needs the F16 activation"
    return Product(mat, x16=x16)


def step_launches(model, x16, bufs, family, wo_prequantised):
    """the four GEMV launches of ONE decode step of a one-layer model, each from the inputs the device had.  x16: the layer input the test
    wrote; bufs: the device's "att", "attq", "a", "t1" after the step (bytes); family: the input family of x16 (decides which
    prologue launches are exactly comparable); wo_prequantised: the plan of the Wo launch reads the attention's quantised image
    (norm == 2).  Returns {role: Launch} for qkv, wo, ffn13, w2."""
    c, M = model.cfg, model.mats
    f16 = lambda name: np.ascontiguousarray(bufs[name]).view(np.float16).reshape(-1)
    par = bool(c.get("parallel_attn", 0) or c.get("share_input", 0))
    out = {}
    # QKV: the normalised, quantised layer input through Wq | Wk | Wv
    xn = _norm(model, x16, "attn_norm")
    xq = q8_image(xn)
    out["qkv"] = Launch("qkv", [_product(M[k], xn, xq) for k in ("wq", "wk", "wv")], EPI_PLAIN,
                        norm_exact(family, c.get("norm_kind", 0), model.norms.get("attn_norm")) and model.norms.get("attn_norm_b") is None)
    # Wo: the attention output as the device quantised it (or quantises it in the launch), + bias, x attn_out_scale, + the layer input
    qd = c["heads"] * c["head_dim"]
    att = f16("att")
    aq = xq_image_to_q8(bufs["attq"], qd) if wo_prequantised else None
    pre = c.get("attn_out_scale") if _scale_on(c.get("attn_out_scale")) else None
    out["wo"] = Launch("wo", [_product(M["wo"], att, aq)], EPI_PLAIN if par else EPI_RESIDUAL, True, res=None if par else x16, pre=pre)
    # W1 | W3: the FFN input (the attention block's output; the attention's normalised input with parallel attention; the layer input
    # when it is shared) behind the FFN norm.  Parallel attention: the QKV launch stores its normalised input (xn_out) for the FFN; after a
    # step the buffer holds the FINAL norm's output (the lm_head launch stores there too), so the reference takes the oracle's norm and
    # the launch counts as a prologue launch, exact where QKV is
    par_attn = bool(c.get("parallel_attn", 0))
    ff_in = xn if par_attn else (x16 if c.get("share_input", 0) else f16("a"))
    has_norm = model.norms.get("ffn_norm") is not None
    hn = _norm(model, ff_in, "ffn_norm") if has_norm else ff_in
    # the FFN input equals the layer input where the test arranged that (see the GPU test): then the family decides, else never exact
    same_in = np.array_equal(np.ascontiguousarray(ff_in, np.float16).view(np.uint16), np.ascontiguousarray(x16, np.float16).view(np.uint16))
    if par_attn:
        ffn_exact = out["qkv"].exact and not has_norm
    else:
        ffn_exact = (not has_norm) or (same_in and norm_exact(family, c.get("norm_kind", 0), model.norms.get("ffn_norm")) and model.norms.get("ffn_norm_b") is None)
    hq = q8_image(hn)
    glu = "w3" in M
    out["ffn13"] = Launch("ffn13", [_product(M[k], hn, hq) for k in (("w1", "w3") if glu else ("w1",))], EPI_GLU if glu else EPI_ACT, ffn_exact,
                          act_kind=c.get("act_kind", 0))
    # W2: the device's own t1, quantised by the reference quantiser, + bias, x ffn_out_scale, + a (+ the layer input), x out_scale
    t1 = f16("t1")
    out["w2"] = Launch("w2", [_product(M["w2"], t1)], EPI_RESIDUAL, True, res=f16("a"), res2=x16 if par else None,
                       pre=c.get("ffn_out_scale") if _scale_on(c.get("ffn_out_scale")) else None,
                       post=c.get("out_scale") if _scale_on(c.get("out_scale")) else None)
    return out, xn


# ----------------------------------------------------------------------------- the column edges both test files walk
MAXNJ = {dt.Q4_B32T1A: 8, dt.Q4_B32T1B: 8, dt.Q8_B32T2: 6, dt.Q4_B64T1: 4, dt.Q3H_B64T1: 4, dt.Q5_B64T1: 4, dt.Q6_B64T1: 4}
INT8_FORMATS = (dt.Q4_B32T1A, dt.Q4_B32T1B, dt.Q8_B32T2, dt.Q4_B64T1, dt.Q3H_B64T1, dt.Q5_B64T1, dt.Q6_B64T1)
F16X_FORMATS = (dt.F16, dt.Q8_B32T1, dt.Q5_B32T1, dt.Q4_B16, dt.Q3_B32T1A, dt.Q2_B32T1B)


def nj_edges(dtype, nj):
    """the widths of nj blocks per lane where a block can be lost: one block into the last round, one block short of a full round, full"""
    cap = dt.block_capacity(dtype)
    L = 64 * cap
    return ((nj - 1) * L + cap, nj * L - cap, nj * L)


def wide_edges(dtype):
    """[(cols, nj)] of the normalised / gated inputs (QKV, W1 / W3; dim <= 8192): every nj up to 4 (B64 formats: 2), one ragged middle
    width; the smallest legal width is nj 1's first edge.  Q4_B32T1B (the bytes and arithmetic of Q4_B32T1A): the nj ends only."""
    cap = dt.block_capacity(dtype)
    L = 64 * cap
    top = 8192 // L
    njs = (1, top) if dtype == dt.Q4_B32T1B else range(1, top + 1)
    e = [(c, nj) for nj in njs for c in nj_edges(dtype, nj)]
    if dtype != dt.Q4_B32T1B:
        e.append((L + L // 2 + 3 * cap, 2))
    return e


def long_edges(dtype):
    """[(cols, kernel, nj, nchunk)] of the plain inputs (Wo, W2): every nj up to MAXNJ, then the long kernel's first width, a ragged one,
    the 2 -> 3 chunk change (Q8_B32T2 only: no other format has one below 32768 columns, and none reaches 4 chunks) and 32768"""
    cap = dt.block_capacity(dtype)
    L = 64 * cap
    mj = MAXNJ[dtype]
    njs = (1, mj) if dtype == dt.Q4_B32T1B else range(1, mj + 1)
    e = [(c, "classic", nj, 1) for nj in njs for c in nj_edges(dtype, nj)]
    if dtype != dt.Q4_B32T1B:
        e.append((2 * L + L // 2 + 3 * cap, "classic", 3, 1))
    lng = [mj * L + cap, 32768] if dtype == dt.Q4_B32T1B else [mj * L + cap, (mj + 2) * L + L // 2 + 3 * cap, 32768]
    if dtype == dt.Q8_B32T2:
        lng += [24576, 24608]
    for c in sorted(lng):
        nj = -(-(c // cap) // 64)
        e.append((c, "long", nj, -(-nj // mj)))
    return e


def f16x_wide_edges(dtype):
    """widths of the fp16-activation kernel's normalised inputs: around one round of the lanes (F16: 256 chunks of 8 = 2048 columns;
    block formats: 64 blocks) and at 8192, the normalised limit; multiples of 32 (the engine's condition on dim)"""
    cap = max(32, dt.block_capacity(dtype))
    L = lane_round(dtype)
    return sorted({cap, L - cap, L, L + cap, 2 * L + L // 2 + cap, 8192 - cap, 8192})


def f16x_long_edges(dtype):
    return [8192 + max(32, dt.block_capacity(dtype)), 16384, 32768]
