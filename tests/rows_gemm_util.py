"""Reference, cases, faults and assertions for checking the rows GEMM (k_gemm_rows_mfma: csrc/ifa_gemm_rows_mfma.hip, ifa_gemm_rows_mo.hip) launch
by launch at its tile, chunk and K-part edges: tests/test_rows_gemm_ref_cpu.py on the host, tests/test_gpu_rows_gemm_edges.py on the device.

A launch computes  Y[t][n] = sum_k X[t][k] w[n][k]  for the rows n of one to three weight matrices (w: the dequantised HALF of every weight)
and 2..32 token rows t, behind an optional RMS-norm prologue (X = norm(raw) x norm weight, rounded to F16) and followed by + bias, then
res + y (residual) or act(y1) x y3 (gated pair).  The reference (float64 of every element, the oracle's value of every token row, d_ref,
bound), the MO layout in NumPy and check_exact come from tests/prompt_gemm_util.py; the input families, SENSITIVITY, FLIP_ROWS_MAX and
ACT_SLOPE from tests/decode_gemv_util.py.  What is added here:

  * the launch plan as a dict (plan) and the shapes of the device test, chosen from it for the CU count at hand (model_cases);
  * RowsRef: the reference of one launch from the inputs the DEVICE had, the flip term of a norm-fused launch, and the float64 output of the
    launch with one systematic fault (faults) -- the list of docs/rows_gemm_edges.md;
  * check: the assertion of the launch's kind, as a function, so that the CPU test can feed it faulty outputs.

Bounds.  Exact-input launches: every element within max(2 x d_ref, one F16 ulp at |element|) of float64, d_ref = max|oracle - float64| over
the launch.  Norm-fused launches on inputs whose normalised value depends on the last bit of the RMS scale add F x (one F16 ulp of the token
row's largest normalised value) x max|w of the weight row| (the gated pair: through ACT_SLOPE, as tests/decode_gemv_util.py); at most
FLIP_ROWS_MAX of a launch's elements may need the term.  F is measured on the device (docs/rows_gemm_edges.md)."""
import numpy as np

import oracle as o
from inferflow_amd import dtypes as dt, worker as W
from tests import decode_gemv_util as G
from tests import prompt_gemm_util as P
from tests.decode_attn_util import ulp16

SENSITIVITY, FLIP_ROWS_MAX, ACT_SLOPE = G.SENSITIVITY, G.FLIP_ROWS_MAX, G.ACT_SLOPE
PLAIN, RESIDUAL, GLU = P.PLAIN, P.RESIDUAL, P.GLU
F_FLIPS = 1                       # the worst flips a launch needed on MI355X (0, on 387 flip-term launches) plus one (docs/rows_gemm_edges.md)
W_STD, B_STD = 0.055, 0.5
SENTINEL = P.SENTINEL
ROLES = ("qkv", "wo", "w13", "w2")
EPI_OF = dict(qkv=PLAIN, wo=RESIDUAL, w13=GLU, w2=RESIDUAL)


def plan(T, rows, cols, epi=PLAIN, norm=0, mo=1, num_cus=256, visible_cus=None, **over):
    return W.gemm_rows_plan(T, rows, cols, epi, norm, mo, num_cus, visible_cus, **over)


def norm_weight(cols):
    """the RMS weight of every model: 1 and 0.5 alternating in runs of 3 -- powers of two, so the sign family stays exact (+-1 x scale x w
    rounds to +-w whatever the last bit of the scale), and not all ones, so a dropped weight shows"""
    return np.where((np.arange(cols) // 3) % 2 == 0, 1.0, 0.5).astype(np.float16)


def make_rows(family, T, cols, seed, live=None):
    """T F16 input rows.  dense N(0, 1); sign +-1; tail: zero except the columns [live[0], live[1]) (the last chunk, or the last K part)"""
    rng = np.random.default_rng(seed)
    if family == "sign":
        return np.where(rng.integers(0, 2, (T, cols)) == 0, -1.0, 1.0).astype(np.float16)
    x = rng.normal(0, 1, (T, cols)).astype(np.float16)
    if family == "tail":
        lo, hi = live
        x[:, :lo] = 0
        x[:, hi:] = 0
    return x


TAIL_COLS = 2048


def tail_cols(K):
    """the live columns of the tail-only family: the last 2048-column chunk of the row, whole or ragged (the chunk of the 17..32-row and
    tiled 9..16-row geometries; it lies inside the last 4096-column chunk and inside the last K part of every part count)"""
    return (K - 1) // TAIL_COLS * TAIL_COLS, K


# ----------------------------------------------------------------------------- one launch
class RCase:
    """the facts of one launch, in the shape tests/prompt_gemm_util.Ref reads them"""

    def __init__(self, role, dtype, T, K, rows, norm, mo, act_kind=0, bias=False, family="dense", tag=""):
        self.role, self.dtype, self.T, self.K, self.rows = role, dtype, T, K, tuple(rows)
        self.epi, self.norm, self.mo, self.act_kind, self.bias, self.family, self.tag = EPI_OF[role], norm, mo, act_kind, bias, family, tag
        self.N = sum(self.rows)
        self.kernel = 0

    @property
    def id(self):
        return "%s-%s-%s-T%d-K%d-N%s-norm%d%s%s%s" % (self.role, dt.name(self.dtype).lower(), "mo" if self.mo else "tiled", self.T, self.K,
                                                    "+".join(map(str, self.rows)), self.norm, "-bias" if self.bias else "",
                                                    "" if self.family == "dense" else "-" + self.family, "-" + self.tag if self.tag else "")

    @property
    def seed(self):
        return 11 * self.T + 13 * self.K + 31 * self.N + 1000 * self.epi + 77 * self.norm + (500 if self.family == "tail" else 0)

    def token_tile(self):
        return 16

    def plan(self, num_cus=256, visible_cus=None, **over):
        return plan(self.T, self.rows, self.K, self.epi, self.norm, self.mo, num_cus, visible_cus, **over)


class RInputs:
    """mats (P.Mat per set), w3 (gated), X [T][K] F16 (behind a norm prologue: the oracle's normalised rows of raw), res [T][N]"""

    def __init__(self, case, mats, w3, X, res=None, raw=None, norm_w=None, eps=1e-5):
        self.case, self.mats, self.w3, self.res, self.raw, self.norm_w, self.eps = case, mats, w3, res, raw, norm_w, eps
        self.X = np.ascontiguousarray(X, np.float16).reshape(case.T, case.K)


def normed(raw, w, eps=1e-5):
    return o.rmsnorm(np.ascontiguousarray(raw, np.float16), w, None, 0.0, eps)


def synth_inputs(case, p=None):
    """host-made inputs of a launch of this shape: weights N(0, W_STD) quantised by the oracle, biases N(0, B_STD), rows of the case's family"""
    c = case
    rng = np.random.default_rng(c.seed)
    bias = lambda r: rng.normal(0, B_STD, r).astype(np.float16) if c.bias else None
    mats = [P.Mat(c.dtype, _quantized(c.dtype, r, c.K, c.seed + 1 + i), r, c.K, bias(r)) for i, r in enumerate(c.rows)]
    w3 = P.Mat(c.dtype, _quantized(c.dtype, c.rows[0], c.K, c.seed + 9), c.rows[0], c.K, bias(c.rows[0])) if c.epi == GLU else None
    raw = make_rows(c.family, c.T, c.K, c.seed + 20, tail_cols(c.K))
    res = rng.normal(0, 1, (c.T, c.N)).astype(np.float16) if c.epi == RESIDUAL else None
    if c.norm or c.role == "qkv":          # (QKV behind the norm launch: the device test rebuilds its input with the oracle's norm too)
        nw = norm_weight(c.K)
        return RInputs(c, mats, w3, normed(raw, nw), res, raw=raw, norm_w=nw)
    return RInputs(c, mats, w3, raw, res)


def _quantized(dtype, rows, cols, seed):
    rng = np.random.default_rng(seed)
    return o.quantize(dtype, rng.normal(0, W_STD, (rows, cols)).astype(np.float16))


def scale_independent(raw, norm_w):
    """True if the normalised F16 rows do not depend on the last bits of the RMS scale: +-1 (or 0) inputs and power-of-two weights"""
    r = np.abs(np.asarray(raw, np.float32))
    w = np.asarray(norm_w, np.float32)
    return bool(np.all((r == 1.0) | (r == 0.0)) and np.all(np.exp2(np.round(np.log2(w))) == w))


class RowsRef(P.Ref):
    """P.Ref of one rows GEMM launch (float64 of every element, the oracle's value of every token row, d_ref, bound) with the flip term of
    a norm-fused launch and the faults.  exact: the input rows are the device's own bit for bit, or do not depend on the device's norm."""

    def __init__(self, inputs):
        super().__init__(inputs)
        c = self.case
        assert len(self.rows) == c.T, "the oracle's value of every token row"
        # (raw: the rows were normalised on the host -- the norm prologue, or a norm launch whose output the step does not keep)
        self.exact = inputs.raw is None or scale_independent(inputs.raw, inputs.norm_w)

    def flip_extra(self, F):
        """float64 [T][N]: what F last-bit differences of the normalised activations may add (0 for an exact launch)"""
        c, I = self.case, self.inp
        if self.exact or F == 0:
            return np.zeros(self.f64.shape)
        xu = ulp16(np.abs(I.X.astype(np.float64)).max(axis=1))[:, None]                   # [T][1]
        wmax = lambda m: np.abs(m.w64).max(axis=1)[None, :]
        if c.epi == GLU:
            d1, d3 = F * xu * wmax(I.mats[0]), F * xu * wmax(I.w3)
            b1 = I.mats[0].bias.astype(np.float64)[None, :] if I.mats[0].bias is not None else 0.0
            b3 = I.w3.bias.astype(np.float64)[None, :] if I.w3.bias is not None else 0.0
            a1, t3 = np.abs(G.act_f64(self.pre[0] + b1, c.act_kind)), np.abs(self.pre3 + b3)
            return ACT_SLOPE * d1 * t3 + a1 * d3 + ACT_SLOPE * d1 * d3
        return F * xu * np.concatenate([wmax(m) for m in I.mats], axis=1)

    def total_bound(self, F):
        return self.bound + self.flip_extra(F)

    # -- faults
    def _cols(self, mat, a, b, X=None):
        X = self.inp.X if X is None else X
        return X[:, a:b].astype(np.float64) @ mat.w64[:, a:b].T

    def _with_x(self, X16):
        """float64 output on other activation rows"""
        I = self.inp
        X64 = np.asarray(X16, np.float16).astype(np.float64)
        return self.finish64([X64 @ m.w64.T for m in I.mats], X64 @ I.w3.w64.T if I.w3 is not None else None)

    def faults(self, p):
        """yields (name, float64 [T][N]) of the launch with one systematic fault; p: the launch's plan (chunks, K parts, rows staged)"""
        c, I = self.case, self.inp
        m0 = I.mats[0]
        K, T, cc, nchunk = c.K, c.T, p["chunk_cols"], p["nchunk"]
        nsup = K // 128
        kp = p["tries"][0]["kparts"]
        kpm, gtiles = p["tries"][0]["kpm"], p["tries"][0]["tiles"]
        part_chunks = nchunk // kp if kp >= 2 else nchunk
        part_cols = [(i * part_chunks * cc, min(K, (i + 1) * part_chunks * cc)) for i in range(kp)] if kp >= 2 else []
        live = np.abs(I.X.astype(np.float64)).sum(axis=0).reshape(nsup, 128).sum(axis=1) > 0            # supersteps with a non-zero activation

        def with0(p0, p3=None):
            return self.finish64([p0] + self.pre[1:], self.pre3 if p3 is None else p3)

        # a 128-column superstep dropped or doubled: the first, the last, the first and last of every chunk and of every K part
        sups = {0, nsup - 1}
        for ch in range(nchunk):
            sups |= {ch * cc // 128, min(nsup, (ch + 1) * cc // 128) - 1}
        for a, b in part_cols:
            sups |= {a // 128, b // 128 - 1}
        for S in sorted(s for s in sups if live[s]):
            d = self._cols(m0, 128 * S, 128 * S + 128)
            yield "superstep %d dropped" % S, with0(self.pre[0] - d)
            yield "superstep %d doubled" % S, with0(self.pre[0] + d)
        if c.epi == GLU and live[nsup - 1]:
            yield "last superstep of W3 dropped", with0(self.pre[0], self.pre3 - self._cols(I.w3, K - 128, K))
        # the ragged last chunk skipped, or read at full length (the columns past K: the head of the next token's row on the next weight row)
        if K % cc and nchunk > 1:
            a = (nchunk - 1) * cc
            yield "ragged last chunk skipped", with0(self.pre[0] - self._cols(m0, a, K))
            over = cc - (K - a)
            Xn, wn = np.roll(I.X, -1, axis=0)[:, :over].astype(np.float64), np.roll(m0.w64, -1, axis=0)[:, :over]
            if Xn.any():                                                   # (tail-only rows begin with zeros: nothing to see there, the dense model of the same K shows it)
                yield "ragged last chunk read at full length", with0(self.pre[0] + Xn @ wn.T)
        # K parts: a part's sum lost, added twice, added to the neighbouring tile of its group, a stale granule of another launch added
        for i, (a, b) in enumerate(part_cols):
            if not live[a // 128:b // 128].any():
                continue
            Pp = self._cols(m0, a, b)
            yield "part %d of %d lost" % (i, kp), with0(self.pre[0] - Pp)
            yield "part %d of %d twice" % (i, kp), with0(self.pre[0] + Pp)
            if c.N >= 32 and gtiles > 1:
                moved = Pp.copy()
                for g0 in range(0, c.N, 16 * gtiles):                      # within a group: tile j's sum lands on tile j + 1 (the last on the first)
                    g1 = min(c.N, g0 + 16 * gtiles)
                    if g1 - g0 >= 32:
                        moved[:, g0:g1] = np.roll(Pp[:, g0:g1], 16, axis=1)
                yield "part %d added to the neighbouring tile" % i, with0(self.pre[0] - Pp + moved)
            yield "stale granule of part %d added" % i, with0(self.pre[0] + np.roll(Pp, 1, axis=0))      # (the previous launch's value: another token's sum)
        # token rows
        for t in sorted({0, T - 2}):
            y = self.f64.copy()
            y[[t, t + 1]] = y[[t + 1, t]]
            yield "token rows %d and %d exchanged" % (t, t + 1), y
        if p["tx"] > T:                                                    # a staged pad row: zeros through the epilogue
            X0 = I.X.copy()
            X0[T - 1] = 0
            yield "row %d receives a pad row's value" % (T - 1), self._with_x(X0)
        if T > 16:
            y = self.f64.copy()
            n2 = T - 16
            y[:n2], y[16:16 + n2] = self.f64[16:16 + n2], self.f64[:n2]
            yield "the two 16-column halves swapped", y
        # a (base, scale) word from the neighbouring superstep / the zero pad of the last quad
        if c.dtype in P.NIBBLE_FORMATS:
            q, base, scale = P.codes_and_words(c.dtype, m0.data, K)
            for S, S2 in ((0, 1), (nsup - 1, nsup - 2), (nsup - 1, None)):
                if (S2 is not None and not (0 <= S2 < nsup and S2 != S)) or not live[S]:
                    continue
                a, b = 128 * S, 128 * S + 128
                w = np.zeros((m0.rows, 128))
                if S2 is not None:
                    for g in range(4):
                        bq = q[:, a + 32 * g:a + 32 * g + 32].astype(np.float32)
                        w[:, 32 * g:32 * g + 32] = (bq * scale[:, 4 * S2 + g:4 * S2 + g + 1] + base[:, 4 * S2 + g:4 * S2 + g + 1]).astype(np.float16).astype(np.float64)
                d = I.X[:, a:b].astype(np.float64) @ (w - m0.w64[:, a:b]).T
                yield "words of superstep %d from %s" % (S, "the zero pad" if S2 is None else "superstep %d" % S2), with0(self.pre[0] + d)
        # sets: the first tile of Wk / Wv from the last tile of the set before it, or with that set's bias
        for i in range(1, len(c.rows)):
            pre = [x.copy() for x in self.pre]
            pre[i][:, :16] = self.pre[i - 1][:, -16:]
            yield "first tile of set %d from the last tile of set %d" % (i, i - 1), self.finish64(pre, None)
            if c.bias:
                bs = [m.bias.copy() for m in I.mats]
                bs[i][:16] = I.mats[i - 1].bias[-16:]
                yield "first tile of set %d with the bias of set %d" % (i, i - 1), self.finish64(self.pre, None, biases=bs)
        if c.epi == GLU:
            yield "W1 and W3 swapped", self.finish64(self.pre, self.pre3, swap_glu=True)
            if c.N >= 32:
                yield "W1's tile i paired with W3's tile i + 1", self._glu_shifted()
        if c.epi == RESIDUAL:
            yield "residual dropped", self.finish64(self.pre, None, res_times=0.0)
            yield "residual doubled", self.finish64(self.pre, None, res_times=2.0)
            yield "residual of the neighbouring token", self.finish64(self.pre, None, res=np.roll(I.res, -1, axis=0))
        if c.bias:
            yield "bias dropped", self.finish64(self.pre, self.pre3, bias=0.0)
        if I.raw is not None:
            yield "norm weight dropped", self._with_x(normed(I.raw, None, I.eps))
            # the RMS over the first chunk only: a norm-fused row is ONE chunk, so the fault is a sum that stops early -- after the first
            # half of the row's columns (2048 of 4096: the other geometry's chunk)
            # (the sign family has the same mean square over any columns: the fault is invisible there by construction and is shown on
            #  the dense model of the same shape)
            half = max(128, K // 2 // 128 * 128)
            if half < K and not self.exact:
                r32 = I.raw.astype(np.float32)
                s_all = 1.0 / np.sqrt((r32.astype(np.float64) ** 2).mean(axis=1) + I.eps)
                s_half = 1.0 / np.sqrt((r32[:, :half].astype(np.float64) ** 2).mean(axis=1) + I.eps)
                ok = np.isfinite(s_half)
                ratio = np.where(ok, s_half / s_all, 0.0)[:, None]
                yield "RMS over the first half of the row only", self._with_x((I.X.astype(np.float64) * ratio).astype(np.float16))

    def _glu_shifted(self):
        c, I = self.case, self.inp
        b3 = I.w3.bias.astype(np.float64)[None, :] if I.w3.bias is not None else 0.0
        b1 = I.mats[0].bias.astype(np.float64)[None, :] if I.mats[0].bias is not None else 0.0
        return G.act_f64(self.pre[0] + b1, c.act_kind) * np.roll(self.pre3 + b3, -16, axis=1)


# ----------------------------------------------------------------------------- the assertion on a device output
def flips_needed(out16, ref, fmax=16):
    """per element: the smallest F >= 0 with |out - float64| <= bound + flip_extra(F) (fmax + 1: none up to fmax)"""
    err = np.abs(np.asarray(out16).astype(np.float64).reshape(ref.f64.shape) - ref.f64)
    need = np.full(ref.f64.shape, fmax + 1, np.int64)
    for F in range(fmax, -1, -1):
        need[err <= ref.total_bound(F)] = F
    return need


def violations(out16, ref, F=F_FLIPS):
    a = np.asarray(out16).astype(np.float64).reshape(ref.f64.shape)
    err = np.abs(a - ref.f64)
    over = int((~(err <= ref.total_bound(0 if ref.exact else F))).sum())
    if not ref.exact and float((err > ref.bound).mean()) > FLIP_ROWS_MAX:
        over = max(over, 1)
    return over


def check(out16, ref, F=F_FLIPS):
    """exact launch: P.check_exact.  Norm-fused launch on scale-dependent inputs: every element within the exact bound + F flips, at most
    FLIP_ROWS_MAX of the elements beyond the exact bound.  Returns (median, worst err / exact bound, share on the flip term, most flips)"""
    if ref.exact:
        med, worst = P.check_exact(out16, ref)
        return med, worst, 0.0, 0
    a = np.asarray(out16).astype(np.float64)
    assert a.shape == ref.f64.shape, (ref.case.id, a.shape, ref.f64.shape)
    assert np.isfinite(a).all(), "%s: output is not finite" % ref.case.id
    err = np.abs(a - ref.f64)
    tb = ref.total_bound(F)
    w = np.unravel_index(int((err - tb).argmax()), err.shape)
    assert (err <= tb).all(), "%s: token %d row %d is %.3g from float64, bound %.3g + %d flips %.3g (%d of %d elements over)" % (
        ref.case.id, w[0], w[1], err[w], ref.bound[w], F, tb[w] - ref.bound[w], int((err > tb).sum()), err.size)
    r = err / ref.bound
    share = float((r > 1.0).mean())
    assert share <= FLIP_ROWS_MAX, "%s: %.2f %% of the elements need the flip term (at most %.1f %%)" % (ref.case.id, 100 * share, 100 * FLIP_ROWS_MAX)
    return float(np.median(r)), float(r.max()), share, int(flips_needed(out16, ref).max())


def perturbed_inputs(inp):
    """the inputs of a norm-fused launch with the fp32 RMS scale one ulp down and one ulp up: what a device whose sum of squares differs in
    the last bit multiplies (tests/decode_gemv_util.perturbed_norms, with the norm weight)"""
    raw = inp.raw.astype(np.float32)
    scale = (np.float32(1.0) / np.sqrt(np.float32(1) * (raw.astype(np.float64) ** 2).mean(axis=1).astype(np.float32) + np.float32(inp.eps), dtype=np.float32)).astype(np.float32)
    w = inp.norm_w.astype(np.float32)[None, :]
    for s in (np.nextafter(scale, np.float32(0)), np.nextafter(scale, np.float32(2) * scale)):
        yield o.f2h((raw * s[:, None]) * w)


# ----------------------------------------------------------------------------- the models of the device test
class ModelCase:
    """a one-layer model (dim, heads x head_dim, kv_heads, ffn), weight format, layout option rows_mo, biases, the step sizes n (the first the
    largest) and the input family of its embedding rows"""

    def __init__(self, group, wd, mo, dim, heads, kv_heads, head_dim, ffn, ns, bias=False, family="dense", kparts=1, tag=""):
        self.group, self.wd, self.mo, self.dim, self.heads, self.kv_heads, self.head_dim, self.ffn = group, wd, mo, dim, heads, kv_heads, head_dim, ffn
        self.ns, self.bias, self.family, self.kparts, self.tag = tuple(ns), bias, family, kparts, tag
        self.qd, self.kvd = heads * head_dim, kv_heads * head_dim

    @property
    def id(self):
        return "%s-%s-%s-d%d-q%d-kv%d-f%d%s%s%s%s" % (self.group, dt.name(self.wd).lower(), "mo" if self.mo else "tiled", self.dim, self.qd, self.kvd, self.ffn,
                                                      "-bias" if self.bias else "", "" if self.family == "dense" else "-" + self.family,
                                                      "" if self.kparts else "-nokparts", "-" + self.tag if self.tag else "")

    def norm_fused(self, n):
        return n <= 8 or (self.mo and n <= 16)            # rule B4 of the batched step's route

    def launches(self, n):
        """{role: RCase} of a step of n rows"""
        nf = int(self.norm_fused(n))
        kw = dict(mo=self.mo, bias=self.bias)
        fam = self.family
        return dict(qkv=RCase("qkv", self.wd, n, self.dim, (self.qd, self.kvd, self.kvd), nf, family=fam, **kw),
                    wo=RCase("wo", self.wd, n, self.qd, (self.dim,), 0, family="tail" if fam == "tail" else "dense", **kw),
                    w13=RCase("w13", self.wd, n, self.dim, (self.ffn,), nf, **kw),
                    w2=RCase("w2", self.wd, n, self.ffn, (self.dim,), 0, family="tail" if fam == "tail" else "dense", **kw))


PROMPT_TOKENS = (2, 8, 9, 16, 17, 32, 40)


def prompt_model(mo):
    """the model of the device test's prompts (forward of PROMPT_TOKENS tokens; 40: 32 + 8, two passes)"""
    return ModelCase("prompt", dt.Q4_B32T1A, mo, 256, 8, 4, 32, 4352, (32,), bias=True)


def prompt_passes(T):
    """[(first token, rows)] of the passes of a T-token prompt on the rows route"""
    return [(0, 32), (32, T - 32)] if T > 32 else [(0, T)]


def heads_for(total, at_least=True):
    """(heads, kv_heads, head_dim) of the smallest QD + 2 KVD >= total a model can have: QD % 128 == 0, kv_heads = heads / 1, 2 or 4,
    head_dim 32, 64 or 128"""
    best = None
    for hd in (128, 64, 32):
        for div, num, den in ((1, 3, 1), (2, 2, 1), (4, 3, 2)):
            unit = hd * num                                              # QD + 2 KVD = heads x hd x num / den
            h = -(-total * den // unit)
            while h % div or (h * hd) % 128:
                h += 1
            t = h * hd * num // den
            if best is None or t < best[0]:
                best = (t, h, h // div, hd)
    return best[1:]


def qkv_total(h, k, hd):
    return (h + 2 * k) * hd


def model_cases(num_cus=256):
    A, B64, Q3H = dt.Q4_B32T1A, dt.Q4_B64T1, dt.Q3H_B64T1
    c = []
    # token rows: every count of rows staged, both layouts (17 and 32: MO only); biases on every matrix; the sign family makes QKV exact
    for fam in ("dense", "sign"):
        c.append(ModelCase("rows", A, 1, 256, 8, 8, 32, 256, (32, 17, 16, 9, 8, 5, 4, 3, 2), bias=True, family=fam))
        c.append(ModelCase("rows", A, 0, 256, 8, 8, 32, 256, (16, 9, 8, 5, 4, 3, 2), bias=True, family=fam))
    for d in (B64, Q3H):
        c.append(ModelCase("rows", d, 1, 256, 8, 8, 32, 256, (32, 16, 9, 8, 2), bias=True))
    # tiles per workgroup through the QKV launch (dim 128): a whole round of the CUs and the first count a model can have past it, for
    # 1 .. 8 rounds and past 8 (the workgroups queue); the set boundaries fall inside a workgroup's tiles from two tiles per workgroup on
    for rounds in (1, 2, 3, 4, 6, 8):
        for extra in (0, 1):
            h, k, hd = heads_for(16 * num_cus * rounds + 16 * extra)
            for mo, ns in ((1, (20, 12, 3)), (0, (12, 3))):
                c.append(ModelCase("tiles", A, mo, 128, h, k, hd, 128, ns, tag="r%d%s" % (rounds, "+" if extra else "")))
    # gated pairs through the W1 / W3 launch (dim 128): 1 .. 4 pairs per workgroup and past 4; norm-fused, separate-norm and 17..32-row forms
    for ffn in sorted({128, 16 * num_cus, 16 * num_cus + 128, 32 * num_cus, 32 * num_cus + 128, 48 * num_cus, 48 * num_cus + 128, 64 * num_cus + 128}):
        c.append(ModelCase("gated", A, 1, 128, 4, 4, 32, ffn, (20, 12, 4), bias=(ffn == 128)))
        c.append(ModelCase("gated", A, 0, 128, 4, 4, 32, ffn, (12, 4)))
    # K of the normalised inputs: one chunk against the chunk loop
    for dim in (2048, 2176, 3968, 4096):
        c.append(ModelCase("kdim", A, 1, dim, 4, 4, 32, 128, (20, 16, 2)))
        c.append(ModelCase("kdim", A, 0, dim, 4, 4, 32, 128, (12, 8)))
    # K of the plain inputs (Wo: QD, W2: ffn): one chunk, the chunk loop, whole rows (MO, n <= 4), K parts (MO, n >= 9)
    for qd, ffn in ((4096, 4224), (4224, 8192), (8192, 11008), (11008, 4096), (16384, 16512)):
        c.append(ModelCase("klong", A, 1, 128, qd // 128, qd // 128, 128, ffn, (32, 17, 16, 9, 4, 2)))
        c.append(ModelCase("klong", A, 0, 128, qd // 128, qd // 128, 128, ffn, (16, 4)))
    c.append(ModelCase("klong", B64, 1, 128, 33, 33, 128, 11008, (17, 9, 4)))
    c.append(ModelCase("klong", Q3H, 1, 128, 33, 33, 128, 11008, (17, 9, 4)))
    # K parts: 2, 3, 4, 6, 8 parts; 5 and 7 chunks (no part count: the plain loop); 9 chunks (3 parts of 3); Wo and W2 with different counts
    for qd, ffn in ((8192, 12288), (16384, 24576), (32768, 20480), (28672, 36864)):
        c.append(ModelCase("kparts", A, 1, 128, qd // 128, qd // 128, 128, ffn, (32, 17, 16, 9), bias=(qd == 8192)))
    c.append(ModelCase("kparts", A, 1, 128, 64, 64, 128, 12288, (32, 16), kparts=0))
    # tail-only: the embedding rows, att and t1 are zero except their last 2048 columns (the device test zeroes the rows of Wv, W1 and W3 in
    # front of them), so a lost last chunk, last part or ragged end cannot hide behind the rest of the sum
    c.append(ModelCase("kparts", A, 1, 128, 64, 64, 128, 11008, (32, 17, 16, 9, 4), family="tail"))
    c.append(ModelCase("kdim", A, 1, 4096, 4, 4, 32, 128, (20, 16), family="tail"))
    c.append(ModelCase("kdim", A, 0, 4096, 4, 4, 32, 128, (12, 8), family="tail"))
    # dim 4096: the most parts the CUs allow; the QKV launch at 17..32 rows past one tile per workgroup (KPM 2)
    # (no matrix past 4096 x 4096: Wo and W2 have 256 tiles and K 4096, two 2048-column chunks at 17..32 rows -- two parts of 128 groups,
    # the most 256 CUs allow)
    c.append(ModelCase("kparts", A, 1, 4096, 32, 8, 128, 4096, (32, 16), tag="wide"))
    return c
