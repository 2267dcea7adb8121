"""Reference, inputs, layouts and assertions for checking the fused prompt GEMM launches (k_gemm_mid, k_gemm_big) at their tile, band,
part and cap edges; tests/test_prompt_gemm_ref_cpu.py exercises all of it on the host.  The device test that applies them does not exist
yet (docs/prompt_gemm_edges.md, "Remaining gaps").

One fused prompt GEMM launch computes  Y[t][n] = sum_k X[t][k] w[n][k]  for the rows n of one to three weight matrices, w being the
dequantised HALF of every weight (half(q x scale + base)), followed by its epilogue: + bias, then res + y (residual) or
act(y1) x y3 (gated pair).  What lives here:

  * the cases both test files walk (mid_cases, big_cases) and their inputs (make_inputs: weights N(0, 0.05) quantised by the oracle,
    activations and residual F16 N(0, 1), biases N(0, 0.5); the tail-only family: activations zero except the last 64-column step of every
    part of K; seeds fixed per shape);
  * the reference of one launch (Ref): the float64 value of EVERY output element (no rounding anywhere) and the oracle's value -- fp32
    sums per token through oracle.gemv_f16x, bias / residual / activation / gate as half operations in the order oracle.Model applies
    them -- of every token row, or on the largest launches of the rows at every 8-row band edge plus the first and the last (oracle_rows);
  * the mutations: the float64 output of a launch with one systematic fault (a K step dropped or doubled, the halves of a superstep
    swapped, a (base, scale) word from the neighbouring superstep or the zero pad, a part of K lost or doubled, a token band or row or
    weight tile from the wrong place, a set boundary moved, the gated halves swapped, the residual or bias wrong);
  * the MO layout ("MFMA operand order", csrc/ifa_gemm_rows_mfma.h) and the Q4_B32T1A-layout copy of the 64-weight formats built in
    NumPy, and the MO copy decoded back by the kernel's own address arithmetic;
  * the assertions a device test applies (check_exact, check_sentinel), as functions, so that the CPU test can feed them mutated outputs.

Tolerance: every element within max(2 x d_ref, one F16 ulp at |element|) of float64, d_ref = max|oracle - float64| over the oracle rows
of the launch (docs/decode_attention_edges.md: the distance of the reference's own rounding points from exact math, times 2 for another
order of the fp32 sums).  The inputs are exact (no device quantiser on this path), so there is no flip term and the slope constant of
tests/decode_gemv_util.py's gated bound never enters: the gated pair has the same bound on its final value."""
import ctypes as C

import numpy as np

import oracle as o
import inferflow_amd as ia
from inferflow_amd import dtypes as dt
from tests.decode_attn_util import ulp16
from tests.decode_gemv_util import SENSITIVITY, act_f64

MID, BIG = 1, 2                           # GmKernel: k_gemm_mid, k_gemm_big
PLAIN, RESIDUAL, GLU = 0, 1, 2
W_STD, B_STD = 0.05, 0.5
NIBBLE_FORMATS = (dt.Q4_B32T1A, dt.Q4_B32T1B, dt.Q4_B64T1, dt.Q3H_B64T1)
SENTINEL = 0x7BCD                         # F16 60832: no product of these inputs comes near it
PAD_ROWS, PAD_COLS = 8, 16


# ----------------------------------------------------------------------------- the plans
MID_FACTS = ("T", "nsets", "rows0", "rows1", "rows2", "nblk", "epi", "num_cus", "no_waits", "waits_on", "max_parts", "ta", "min_steps",
             "two_per_cu", "no_glu_split", "mo", "has_w1", "ld_or")
BIG_FACTS = ("T", "nsets", "rows0", "rows1", "rows2", "nblk", "dtype", "epi", "tiles_bits", "num_cus", "no_waits", "waits_on", "has_w1", "ld_or")
LAUNCH_FIELDS = ("bm", "bn", "waves", "tn0", "tn_count", "tiles_m", "lds")


def _rows3(rows):
    rows = tuple(rows)
    return rows + (0,) * (3 - len(rows))


def mid_plan(T, rows, cols, epi=PLAIN, num_cus=256, **over):
    """ifa_gemm_mid_plan as a dict: error, ta, tiles_m, tiles_n, tile0, ksteps, tries = [(parts, grid, lds)] in the order they are tried"""
    f = dict(T=T, nsets=len(rows), nblk=cols // 32, epi=epi, num_cus=num_cus, no_waits=0, waits_on=1, max_parts=0, ta=0, min_steps=0,
             two_per_cu=0, no_glu_split=0, mo=1, has_w1=1, ld_or=0)
    f.update(zip(("rows0", "rows1", "rows2"), _rows3(rows)))
    f.update(over)
    facts = (C.c_int * len(MID_FACTS))(*[int(f[k]) for k in MID_FACTS])
    out = (C.c_int * 25)()
    ia.check(ia.lib().ifa_gemm_mid_plan(facts, len(MID_FACTS), out, 25))
    v = list(out)
    n = v[9]
    return dict(error=v[0], ta=v[1], tiles_m=v[2], tiles_n=v[3], tile0=v[4:8], ksteps=v[8],
                tries=[(v[10 + i], v[15 + i], v[20 + i]) for i in range(n)])


def big_plan(T, rows, cols, dtype=dt.Q4_B32T1A, epi=PLAIN, tiles_bits=1, num_cus=256, **over):
    """ifa_gemm_big_plan as a dict: error, pick, stream_k, launches = [dict of LAUNCH_FIELDS], full_n, rem_n, ks = parts of K in order"""
    cap = 32 if dtype == dt.F16 else dt.block_capacity(dtype)
    f = dict(T=T, nsets=len(rows), nblk=cols // cap, dtype=dtype, epi=epi, tiles_bits=tiles_bits, num_cus=num_cus, no_waits=0, waits_on=1,
             has_w1=1, ld_or=0)
    f.update(zip(("rows0", "rows1", "rows2"), _rows3(rows)))
    f.update(over)
    facts = (C.c_int * len(BIG_FACTS))(*[int(f[k]) for k in BIG_FACTS])
    out = (C.c_int * 23)()
    ia.check(ia.lib().ifa_gemm_big_plan(facts, len(BIG_FACTS), out, 23))
    v = list(out)
    return dict(error=v[0], pick=v[1], stream_k=v[2],
                launches=[dict(zip(LAUNCH_FIELDS, v[4 + 7 * i:11 + 7 * i])) for i in range(v[3])],
                full_n=v[18], rem_n=v[19], ks=v[21:21 + v[20]])


def part_steps(ksteps, parts):
    """[(first step, steps)] of every part of K, as k_gemm_mid and k_gemm_big's split-K forms divide them (parts may differ by one step)"""
    return [(kz * ksteps // parts, (kz + 1) * ksteps // parts - kz * ksteps // parts) for kz in range(parts)]


# ----------------------------------------------------------------------------- cases
class Case:
    """one launch: kernel MID / BIG, weight format, tokens T, columns K, rows of each set (gated: row pairs), epilogue, activation kind,
    bias, input family, one output matrix or three, and the launcher's settings; plan_parts: the parts of K the plan takes first on 256
    CUs (the mutations of a part are shown for it; a device test plans for its own device)"""

    def __init__(self, kernel, dtype, T, K, rows, epi=PLAIN, act_kind=0, bias=False, family="dense", one_y=True, no_waits=0, max_parts=0,
                 ta=0, tiles_bits=1, tag=""):
        self.kernel, self.dtype, self.T, self.K, self.rows = kernel, dtype, T, K, tuple(rows)
        self.epi, self.act_kind, self.bias, self.family, self.one_y = epi, act_kind, bias, family, one_y
        self.no_waits, self.max_parts, self.ta, self.tiles_bits, self.tag = no_waits, max_parts, ta, tiles_bits, tag
        self.N = sum(self.rows)

    @property
    def id(self):
        e = ("plain", "res", "glu%d" % self.act_kind)[self.epi]
        s = "%s-%s-T%d-K%d-N%s-%s" % ("mid" if self.kernel == MID else "big", dt.name(self.dtype).lower(), self.T, self.K,
                                      "+".join(map(str, self.rows)), e)
        s += "-bias" if self.bias else ""
        s += "" if self.one_y or len(self.rows) == 1 else "-3y"
        s += "-tail" if self.family == "tail" else ""
        return s + ("-" + self.tag if self.tag else "")

    @property
    def seed(self):
        """fixed per shape"""
        return 7 * self.T + 13 * self.K + 31 * self.N + 1000 * self.epi + (500 if self.family == "tail" else 0)

    def plan(self, num_cus=256, waits_on=1):
        if self.kernel == MID:
            return mid_plan(self.T, self.rows, self.K, self.epi, num_cus, no_waits=self.no_waits, max_parts=self.max_parts, ta=self.ta,
                            waits_on=waits_on)
        d = dt.Q4_B32T1A if self.dtype in (dt.Q4_B64T1, dt.Q3H_B64T1) else self.dtype       # (the expanded copy)
        return big_plan(self.T, self.rows, self.K, d, self.epi, self.tiles_bits, num_cus, no_waits=self.no_waits, waits_on=waits_on)

    def parts(self, num_cus=256):
        p = self.plan(num_cus)
        return p["tries"][0][0] if self.kernel == MID else p["ks"][0]

    def token_tile(self):
        if self.kernel == MID:
            return 256 if self.ta == 8 else 128
        return self.plan()["launches"][0]["bm"]


MID_T = (1, 8, 33, 47, 48, 49, 127, 128, 129, 160, 257)
MID_K = (256, 512, 640, 768, 896, 1024, 1152, 2048, 2176, 4224)
MID_K_FORMATS = (640, 1152, 2176)


def cap_edge_rows(K=2048, T=33, num_cus=256):
    """the smallest N (one set, plain) at which the workgroup cap of `num_cus` drops the first choice from 8 parts to 4 at K columns, and
    that N less one tile -- chosen from the plan"""
    n = 128
    while mid_plan(T, (n,), K, PLAIN, num_cus)["tries"][0][0] == 8:
        n += 128
    return n, n - 128


def mid_cases(num_cus=256):
    A = dt.Q4_B32T1A
    c = []
    # every K at 33 and 129 tokens with one and three sets
    for T in (33, 129):
        for K in MID_K:
            c.append(Case(MID, A, T, K, (144,), PLAIN, bias=True))
            c.append(Case(MID, A, T, K, (64, 16, 16), PLAIN, bias=True, one_y=(T == 33)))
    # every token count at 640 and 2176 columns
    for T in MID_T:
        for K in (640, 2176):
            c.append(Case(MID, A, T, K, (112,), RESIDUAL, bias=(K == 640)))
    # rows and sets
    for n in (16, 112, 128, 144):
        c.append(Case(MID, A, 47, 1152, (n,), PLAIN))
    for rows in ((128, 128, 128), (64, 16, 16), (192, 48, 48)):
        for one_y in (True, False):
            c.append(Case(MID, A, 49, 1024, rows, PLAIN, bias=True, one_y=one_y))
    for n in (16, 64, 80, 192):
        c.append(Case(MID, A, 48, 896, (n,), GLU, act_kind=0, bias=(n == 80)))
    # each epilogue
    c.append(Case(MID, A, 160, 768, (128,), PLAIN, bias=False))
    c.append(Case(MID, A, 160, 768, (128,), PLAIN, bias=True))
    c.append(Case(MID, A, 160, 768, (128,), RESIDUAL, bias=True))
    for kind in (0, 1, 2):
        c.append(Case(MID, A, 127, 512, (80,), GLU, act_kind=kind, bias=True))
    # the other formats
    for d in (dt.Q4_B32T1B, dt.Q4_B64T1, dt.Q3H_B64T1):
        for K in MID_K_FORMATS:
            c.append(Case(MID, d, 129, K, (64, 16, 16), PLAIN, bias=True, one_y=False))
            c.append(Case(MID, d, 49, K, (80,), GLU, act_kind=0))
            c.append(Case(MID, d, 33, K, (48,), RESIDUAL))
    # tail-only inputs
    for K in (640, 1152, 2176):
        c.append(Case(MID, A, 33, K, (144,), PLAIN, family="tail"))
        c.append(Case(MID, A, 129, K, (112,), RESIDUAL, family="tail"))
    # no_waits at 2048 columns: one part on the long K
    c.append(Case(MID, A, 129, 2048, (144,), RESIDUAL, no_waits=1, tag="nowaits"))
    # the cap of the device drops eight parts to four
    n4, n8 = cap_edge_rows(2048, 33, num_cus)
    c.append(Case(MID, A, 33, 2048, (n4,), PLAIN, tag="cap4"))
    c.append(Case(MID, A, 33, 2048, (n8,), PLAIN, tag="cap8"))
    # the measurement instances
    c.append(Case(MID, A, 257, 1152, (144,), RESIDUAL, ta=8, tag="ta8"))
    c.append(Case(MID, A, 48, 4096, (112,), PLAIN, max_parts=16, tag="ks16"))
    return c


def two_launch_rows(T=256, K=256, num_cus=256):
    """the smallest N (one set, plain, Q4_B32T1A) whose automatic plan is the two-launch form at T tokens"""
    n = 256
    while True:
        p = big_plan(T, (n,), K, num_cus=num_cus)
        if len(p["launches"]) == 2:
            return n
        n += 256
        assert n < (1 << 20)


def big_cases(num_cus=256):
    A, Q8 = dt.Q4_B32T1A, dt.Q8_B32T2
    c = []
    for force in (1, 2, 3, 4, 5, 6):
        bits = 1 | (force << 8)
        T, rows, K = ((150, 136, 2112), (257, 264, 192), (150, 520, 192), (257, 136, 192), (150, 264, 2112), (257, 520, 192))[force - 1]
        c.append(Case(BIG, A, T, K, (rows,), RESIDUAL, bias=True, tiles_bits=bits, tag="f%d" % force))
        c.append(Case(BIG, A, T, K, (rows,), GLU, act_kind=0, tiles_bits=bits, tag="f%d" % force))
        c.append(Case(BIG, A, T, K, (rows, 136, 136), PLAIN, bias=True, one_y=False, tiles_bits=bits, tag="f%d" % force))
        c.append(Case(BIG, Q8, T, K, (rows,), PLAIN, bias=True, tiles_bits=bits, tag="f%d" % force))
    f3 = 1 | (3 << 8)
    for d in (dt.Q5_B32T1, dt.Q4_B16, dt.F16, dt.Q3H_B64T1, dt.Q4_B64T1):
        c.append(Case(BIG, d, 150, 192, (136,), PLAIN, bias=True, tiles_bits=f3, tag="f3"))
    c.append(Case(BIG, dt.Q3H_B64T1, 257, 2112, (264,), RESIDUAL, tiles_bits=f3, tag="f3"))
    c.append(Case(BIG, dt.Q4_B64T1, 150, 2112, (136,), GLU, tiles_bits=f3, tag="f3"))
    # the automatic choice
    c.append(Case(BIG, A, 256, 2048, (64 * 128,), RESIDUAL, tag="splitk2"))
    c.append(Case(BIG, Q8, 256, 2048, (64 * 128,), PLAIN, tag="splitk2"))
    for T in (48, 128):
        c.append(Case(BIG, A, T, 4096, (128,), RESIDUAL, bias=True, tag="splitk4"))
    c.append(Case(BIG, Q8, 128, 4096, (128,), PLAIN, tag="splitk4"))
    c.append(Case(BIG, A, 513, 256, (128,), RESIDUAL, tag="w4"))
    n2 = two_launch_rows(129, 256, num_cus)      # (one 256-token tile, two of 128 tokens in the second launch)
    c.append(Case(BIG, A, 129, 256, (n2,), RESIDUAL, bias=True, tag="two"))
    c.append(Case(BIG, A, 130, 256, (n2 // 2,), GLU, tag="two"))
    return c


# ----------------------------------------------------------------------------- weights
class Mat:
    """one weight matrix in the reference byte layout with the float64 view of its dequantised halves"""

    def __init__(self, dtype, data, rows, cols, bias=None):
        self.dtype, self.rows, self.cols = dtype, rows, cols
        self.bias = None if bias is None else np.ascontiguousarray(bias, np.float16).reshape(-1)
        if dtype == dt.F16:
            self.data = np.ascontiguousarray(data).view(np.float16).reshape(rows, cols)
            self.w64 = self.data.astype(np.float64)
        else:
            self.data = np.ascontiguousarray(data, np.uint8).reshape(rows, dt.row_bytes(dtype, cols))
            self.w64 = o.dequantize(dtype, self.data, cols).astype(np.float64)


def quantized(dtype, rows, cols, seed):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, W_STD, (rows, cols)).astype(np.float16)
    return w if dtype == dt.F16 else o.quantize(dtype, w)


def tail_columns(K, parts):
    """the columns of the last 64-column step of every part of K"""
    return [(64 * (s0 + n - 1), 64 * (s0 + n)) for s0, n in part_steps(K // 64, parts)]


class Inputs:
    def __init__(self, case, parts=None):
        c = self.case = case
        rng = np.random.default_rng(c.seed)
        self.mats = [Mat(c.dtype, quantized(c.dtype, r, c.K, c.seed + 1 + i), r, c.K,
                         rng.normal(0, B_STD, r).astype(np.float16) if c.bias else None) for i, r in enumerate(c.rows)]
        self.w3 = None
        if c.epi == GLU:
            self.w3 = Mat(c.dtype, quantized(c.dtype, c.rows[0], c.K, c.seed + 9), c.rows[0], c.K,
                          rng.normal(0, B_STD, c.rows[0]).astype(np.float16) if c.bias else None)
        X = rng.normal(0, 1, (c.T, c.K)).astype(np.float16)
        if c.family == "tail":
            keep = np.zeros(c.K, bool)
            for lo, hi in tail_columns(c.K, parts if parts is not None else c.parts()):
                keep[lo:hi] = True
            X[:, ~keep] = 0
        self.X = X
        self.res = rng.normal(0, 1, (c.T, c.N)).astype(np.float16) if c.epi == RESIDUAL else None


# ----------------------------------------------------------------------------- the reference
ORACLE_ALL_WORK = 1.5e9


def oracle_rows(T, work=None):
    """the token rows whose oracle value is computed.  d_ref is the maximum over the LAUNCH, so every row where that is affordable
    (tokens x rows x columns <= ORACLE_ALL_WORK multiply-adds of the scalar oracle); above that both sides of every 8-row band edge
    (which covers every tile edge), the first and the last row.  (The edge rows alone understate d_ref on small launches: on
    mid-q4_b64t1-T49-K640-N80-glu0 the 13 edge rows give 0.0029, all 49 rows 0.0093 -- the product of two rounded halves has a long
    tail -- and the oracle's own value of token 1, row 46 then lies outside the bound made from it.)"""
    if work is not None and work <= ORACLE_ALL_WORK:
        return np.arange(T)
    r = {0, T - 1}
    for e in range(8, T, 8):
        r.update((e - 1, e))
    return np.array(sorted(r))


class Ref:
    """the reference of one launch: f64 [T][N] (every element, no rounding), orc [len(rows)][N] (the oracle's value of the token rows
    `rows`), d_ref, bound [T][N]"""

    def __init__(self, inputs):
        I = self.inp = inputs
        c = self.case = I.case
        self.rows = oracle_rows(c.T, float(c.T) * c.N * c.K * (2 if c.epi == GLU else 1))
        X64 = I.X.astype(np.float64)
        self.pre = [X64 @ m.w64.T for m in I.mats]                                  # the products, float64
        self.pre3 = X64 @ I.w3.w64.T if I.w3 is not None else None
        self.f64 = self.finish64(self.pre, self.pre3)
        Xr = np.ascontiguousarray(I.X[self.rows])
        ys = [o.gemm_f16x(m.dtype, m.data, m.rows, m.cols, Xr, m.bias) for m in I.mats]
        if c.epi == GLU:
            y3 = o.gemm_f16x(I.w3.dtype, I.w3.data, I.w3.rows, I.w3.cols, Xr, I.w3.bias)
            orc = o.mul(o.act(ys[0], c.act_kind), y3)
        else:
            orc = np.concatenate(ys, axis=1)
            if c.epi == RESIDUAL:
                orc = o.add(np.ascontiguousarray(I.res[self.rows]), np.ascontiguousarray(orc))
        self.orc = np.asarray(orc, np.float16).reshape(len(self.rows), c.N)
        self.d_ref = float(np.abs(self.orc.astype(np.float64) - self.f64[self.rows]).max())
        self.bound = np.maximum(2.0 * self.d_ref, ulp16(self.f64))

    def finish64(self, pre, pre3, bias=1.0, res_times=1.0, res=None, biases=None, swap_glu=False):
        """the epilogue in float64 without rounding; the keyword arguments are the mutations' handles"""
        c, I = self.case, self.inp
        bs = biases if biases is not None else [m.bias for m in I.mats]
        ys = [p + (bias * b.astype(np.float64)[None, :] if b is not None else 0.0) for p, b in zip(pre, bs)]
        if c.epi == GLU:
            y3 = pre3 + (bias * I.w3.bias.astype(np.float64)[None, :] if I.w3.bias is not None else 0.0)
            y1 = ys[0]
            if swap_glu:
                y1, y3 = y3, y1
            return act_f64(y1, c.act_kind) * y3
        y = np.concatenate(ys, axis=1)
        if c.epi == RESIDUAL:
            y = y + res_times * (I.res if res is None else res).astype(np.float64)
        return y

    def device_like(self, delta=None):
        """an F16 output as a correct device would give it -- the oracle's value on the oracle rows, the rounded float64 value elsewhere --
        shifted by delta (float64 [T][N])"""
        out = self.f64.astype(np.float16)
        out[self.rows] = self.orc
        if delta is None:
            return out
        return (out.astype(np.float64) + delta).astype(np.float16)

    # -- mutations
    def _steps(self, mat, lo, n=1):
        """float64 [T][rows]: the contribution of the 64-column steps [lo, lo + n) of `mat`"""
        a, b = 64 * lo, 64 * (lo + n)
        return self.inp.X[:, a:b].astype(np.float64) @ mat.w64[:, a:b].T

    def _cross(self, mat, wstep, xstep):
        """weight columns of step wstep on the activations of step xstep"""
        return self.inp.X[:, 64 * xstep:64 * xstep + 64].astype(np.float64) @ mat.w64[:, 64 * wstep:64 * wstep + 64].T

    def mutations(self, parts):
        """yields (name, float64 [T][N] output) of the launch with one systematic fault; parts: the parts of K of the instance"""
        c, I = self.case, self.inp
        m0 = I.mats[0]
        ksteps = c.K // 64
        ps = part_steps(ksteps, parts)

        def with0(p0, p3=None):
            return self.finish64([p0] + self.pre[1:], self.pre3 if p3 is None else p3)

        # (the tail-only family multiplies every other step by zero: there the steps that count are the last ones of the parts)
        live = {s0 + n - 1 for s0, n in ps} if c.family == "tail" else set(range(ksteps))
        steps = sorted(({0, ksteps - 1} | {s0 for s0, _ in ps} | ({s0 + n - 1 for s0, n in ps} if c.family == "tail" else set())) & live)
        for j in steps:
            S = self._steps(m0, j)
            yield "step %d dropped" % j, with0(self.pre[0] - S)
            yield "step %d doubled" % j, with0(self.pre[0] + S)
        if c.epi == GLU:
            S = self._steps(I.w3, ksteps - 1)
            yield "last step of W3 dropped", with0(self.pre[0], self.pre3 - S)
        # the halves of a superstep swapped (weights of one half on the activations of the other)
        if c.K % 128 == 0:
            odd = [s0 // 2 for s0, _ in ps if s0 % 2]
            for S2 in sorted({0, ksteps // 2 - 1} | set(odd)):
                a, b = 2 * S2, 2 * S2 + 1
                if not ({a, b} & live):
                    continue
                d = self._cross(m0, a, b) + self._cross(m0, b, a) - self._steps(m0, a, 2)
                yield "halves of superstep %d swapped" % S2, with0(self.pre[0] + d)
        # a (base, scale) word from the neighbouring superstep / the zero pad of the last quad
        if c.kernel == MID and c.dtype in NIBBLE_FORMATS:
            nsup = c.K // 128
            q, base, scale = codes_and_words(c.dtype, m0.data, c.K)                   # [rows][K], [rows][K / 32] x 2
            for S, S2 in ((0, 1), (nsup - 1, nsup - 2), (nsup // 2, nsup // 2 + 1), (nsup - 1, None)):
                if (S2 is not None and not (0 <= S2 < nsup and S2 != S)) or not ({2 * S, 2 * S + 1} & live):
                    continue
                w = m0.w64.copy()
                for g in range(4):
                    bq = q[:, 128 * S + 32 * g:128 * S + 32 * g + 32].astype(np.float32)
                    if S2 is None:
                        w[:, 128 * S + 32 * g:128 * S + 32 * g + 32] = 0.0
                    else:
                        sc, ba = scale[:, 4 * S2 + g:4 * S2 + g + 1], base[:, 4 * S2 + g:4 * S2 + g + 1]
                        w[:, 128 * S + 32 * g:128 * S + 32 * g + 32] = (bq * sc + ba).astype(np.float16).astype(np.float64)
                a, b = 128 * S, 128 * S + 128
                d = I.X[:, a:b].astype(np.float64) @ (w[:, a:b] - m0.w64[:, a:b]).T
                yield "words of superstep %d from %s" % (S, "the zero pad" if S2 is None else "superstep %d" % S2), with0(self.pre[0] + d)
        # a part of K lost or added twice; an 8-row band taking the next band's rows
        if parts > 1:
            for kz in sorted({0, parts - 1, parts // 2}):
                P = self._steps(m0, ps[kz][0], ps[kz][1])
                yield "part %d of %d lost" % (kz, parts), with0(self.pre[0] - P)
                yield "part %d of %d twice" % (kz, parts), with0(self.pre[0] + P)
        if c.T > 8:
            y = self.f64.copy()
            src = np.minimum(np.arange(c.T) ^ 8, c.T - 1)
            yield "8-row bands exchanged in pairs", y[src]
        # token rows and weight rows at the clamped edges
        bm = c.token_tile()
        t0 = (c.T - 1) // bm * bm
        if t0 < c.T - 1:
            y = self.f64.copy()
            y[t0] = y[c.T - 1]
            yield "row %d receives row %d's result" % (t0, c.T - 1), y
        off = 0
        for i, r in enumerate(c.rows):
            if r >= 32:
                y = self.f64.copy()
                y[:, off + r - 32:off + r - 16] = y[:, off + r - 16:off + r]
                yield "last 16-row tile of set %d one tile early" % i, y
            off += r
        if len(c.rows) > 1:
            pre = [p.copy() for p in self.pre]
            pre[1][:, 0] = self.pre[0][:, -1]
            yield "first K row from Wq's tail", self.finish64(pre, None)
            if c.bias:
                bs = [m.bias for m in I.mats]
                wrong = np.resize(bs[0], bs[1].size)
                yield "bias of the wrong set", self.finish64(self.pre, None, biases=[bs[0], wrong] + bs[2:])
        if c.epi == GLU:
            yield "W1 / W3 swapped", self.finish64(self.pre, self.pre3, swap_glu=True)
        if c.epi == RESIDUAL:
            yield "residual dropped", self.finish64(self.pre, None, res_times=0.0)
            yield "residual doubled", self.finish64(self.pre, None, res_times=2.0)
            if c.T > 1:
                yield "residual of the neighbouring token", self.finish64(self.pre, None, res=np.roll(I.res, -1, axis=0))
        if c.bias:
            yield "bias dropped", self.finish64(self.pre, self.pre3, bias=0.0)


# ----------------------------------------------------------------------------- the assertions on a device output
def violations(out16, ref):
    a = np.asarray(out16).astype(np.float64).reshape(ref.f64.shape)
    return int((~(np.abs(a - ref.f64) <= ref.bound)).sum())


def check_exact(out16, ref):
    """every element of the launch's output within max(2 x d_ref, one F16 ulp at |element|) of float64; returns (median, worst) err / bound"""
    a = np.asarray(out16).astype(np.float64)
    assert a.shape == ref.f64.shape, (ref.case.id, a.shape, ref.f64.shape)
    assert np.isfinite(a).all(), "%s: output is not finite" % ref.case.id
    r = np.abs(a - ref.f64) / ref.bound
    w = np.unravel_index(int(r.argmax()), r.shape)
    assert r[w] <= 1.0, "%s: token %d row %d is %.3g from float64, bound %.3g (d_ref %.3g; %d of %d elements over)" % (
        ref.case.id, w[0], w[1], abs(a[w] - ref.f64[w]), ref.bound[w], ref.d_ref, int((r > 1.0).sum()), r.size)
    return float(np.median(r)), float(r[w])


def sentinel_frame(T, n, ld):
    """uint16 [T + PAD_ROWS][ld] filled with the sentinel pattern (it varies with the position, so a shifted store shows)"""
    a = (np.arange((T + PAD_ROWS) * ld, dtype=np.uint32) % 251).astype(np.uint16)
    return (SENTINEL + a).reshape(T + PAD_ROWS, ld)


def check_sentinel(frame_after, T, n, ld, name=""):
    """nothing outside [0, T) x [0, n) of an output frame was touched"""
    want = sentinel_frame(T, n, ld)
    got = np.asarray(frame_after).view(np.uint16).reshape(T + PAD_ROWS, ld)
    mask = np.ones(got.shape, bool)
    mask[:T, :n] = False
    bad = mask & (got != want)
    assert not bad.any(), "%s: %d elements outside the output were written, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


# ----------------------------------------------------------------------------- layouts
def codes_and_words(dtype, data, cols):
    """of a nibble format (value = q x scale + base): q int32 [rows][cols], base and scale float32 [rows][cols / 32] (the 64-weight
    formats: the block's word for both of its halves)"""
    data = np.ascontiguousarray(data, np.uint8)
    rows = data.shape[0]
    q = o.unpack_codes(dtype, data, cols)
    cap, bb = dt.block_capacity(dtype), dt.block_bytes(dtype)
    w = data.reshape(rows, cols // cap, bb)[:, :, :4].copy().view(np.float16).astype(np.float32)      # [rows][blocks][base, scale]
    rep = cap // 32
    return q, np.repeat(w[:, :, 0], rep, axis=1), np.repeat(w[:, :, 1], rep, axis=1)


def _nibble_bytes_and_words(dtype, data, cols):
    """uint8 [rows][cols / 32][16] code bytes (byte i = weights 2 i | 2 i + 1 << 4) and uint8 [rows][cols / 32][4] (base, scale) words"""
    data = np.ascontiguousarray(data, np.uint8)
    rows = data.shape[0]
    q = o.unpack_codes(dtype, data, cols).astype(np.uint8)
    nib = (q[:, 0::2] | (q[:, 1::2] << 4)).reshape(rows, cols // 32, 16)
    cap, bb = dt.block_capacity(dtype), dt.block_bytes(dtype)
    words = np.repeat(data.reshape(rows, cols // cap, bb)[:, :, :4], cap // 32, axis=1)
    return nib, words


def mo_bytes(rows, cols):
    nsup = cols // 128
    return (rows + 15) // 16 * (nsup + (nsup + 3) // 4) * 1024


def mo_build_np(dtype, data, rows, cols):
    """the MO copy as csrc/ifa_gemm_rows_mfma.h describes it.  Per tile of 16 rows: nsup = cols / 128 supersteps of 1024 bytes -- lane
    l = 16 g + r owns bytes 16 l .. 16 l + 15, the 16 code bytes of block 4 S + g of row 16 tile + r --, then ceil(nsup / 4) quads of 1024
    bytes -- lane l owns the (base, scale) words of its blocks in supersteps 4 Q .. 4 Q + 3.  Rows past the end and the pad of the last
    quad are zero."""
    nib, words = _nibble_bytes_and_words(dtype, data, cols)
    nsup, ntile = cols // 128, (rows + 15) // 16
    nq4 = (nsup + 3) // 4
    out = np.zeros((ntile, nsup + nq4, 64, 16), np.uint8)
    for row in range(rows):
        tile, r = divmod(row, 16)
        for g in range(4):
            lane = 16 * g + r
            out[tile, :nsup, lane, :] = nib[row, g::4, :]                            # superstep S: block 4 S + g
            wq = np.zeros((nq4 * 4, 4), np.uint8)
            wq[:nsup] = words[row, g::4, :]
            out[tile, nsup:, lane, :] = wq.reshape(nq4, 16)                           # quad Q: supersteps 4 Q .. 4 Q + 3
    return out.reshape(-1)


def mo_decode_np(mo, rows, cols):
    """the dequantised matrix (float16 [rows][cols]) read back from an MO copy with k_gemm_mid's address arithmetic: 16-row tile `tile`,
    64-column step `step` = half h of superstep S; lane (g2, r) of the half reads the 16 code bytes at tile x mo_tile + S x 1024 +
    (16 (2 h + g2) + r) x 16 and the word at tile x mo_tile + (nsup + S / 4) x 1024 + (16 (2 h + g2) + r) x 16 + 4 (S % 4)"""
    mo = np.ascontiguousarray(mo, np.uint8).reshape(-1)
    nsup = cols // 128
    mo_tile = (nsup + (nsup + 3) // 4) * 1024
    out = np.zeros((rows, cols), np.float16)
    for row in range(rows):
        tile, r = divmod(row, 16)
        for step in range(cols // 64):
            S, h = divmod(step, 2)
            for g2 in range(2):
                lane = 16 * (2 * h + g2) + r
                ca = tile * mo_tile + S * 1024 + lane * 16
                wa = tile * mo_tile + (nsup + S // 4) * 1024 + lane * 16 + 4 * (S % 4)
                b = mo[ca:ca + 16]
                q = np.empty(32, np.float32)
                q[0::2], q[1::2] = b & 15, b >> 4
                base, scale = mo[wa:wa + 4].copy().view(np.float16).astype(np.float32)
                out[row, 64 * step + 32 * g2:64 * step + 32 * g2 + 32] = (q * scale + base).astype(np.float16)
    return out


def expand_b64_np(dtype, data, rows, cols):
    """Q4_B64T1 / Q3H_B64T1 rows as Q4_B32T1A reference-layout blocks {base, scale, 16 code bytes} per 32 weights, the 64-block's word in
    both halves"""
    nib, words = _nibble_bytes_and_words(dtype, data, cols)
    return np.concatenate([words, nib], axis=2).reshape(rows, cols // 32 * 20)
