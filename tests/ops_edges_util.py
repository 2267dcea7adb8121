"""The float64 references, the cases, the bounds, the checks and the designed faults of the row-op edge tests
(tests/test_gpu_ops_edges.py runs the launches of csrc/ifa_ops.hip; tests/test_ops_edges_ref_cpu.py proves on the host that the
checks accept the oracle and reject every fault).  docs/prompt_ops_edges.md has the branch map and the recorded figures.

Every bound is (one final F16 rounding) + (the fp32 roundings of the written expression) + (a device-math term).  The device-math
constants are measured HERE, on the host, as libm's error on the same fp32 expression against float64 (`measure_*`; the oracle calls
the same libm), and doubled for the device: a second implementation of powf / cosf / sinf / expf / tanhf in the same documented
accuracy class may err as far again in the other direction.  No constant comes from a device result.

  RoPE       A_ROPE_CPU  = 1.2  x pos x 2^-23 bounds |cosf(ang32) - cos(ang64)| and |sinf ..|, ang32 = pos * powf(powf(theta, -2 / rd), col):
             the relative error of powf(ts, col) is col x the error of ts plus its own, while ts^col shrinks -- col x ts^col peaks
             near 3.4 (theta 1e6, rope_dims 256) -- and cosf / sinf add their own ulp.  Measured 1.137 over every (theta, rope_dims,
             position, pair) of the cases below (`measure_rope`).
  expf       A_EXP_CPU   = 0.51 fp32 ulps of the result: measured 0.5012 over expf(-v), v every finite half (silu; softmax uses the same).
  tanhf      A_TANH_CPU  = 2.2  fp32 ulps of the result: measured 2.123 over the gelu argument of every finite half.
  ALiBi      A_SLOPE_CPU = 6.5  fp32 ulps of the slope powf(powf(2, -8 / hl2), head + 1): the outer powf multiplies the inner one's
             error by head + 1 <= 32.  Measured 6.21 over 8 / 12 / 16 / 40 heads (`measure_slope`).
tests/test_ops_edges_ref_cpu.py re-measures all four and fails when one exceeds its constant.
"""
import ctypes as C
import ctypes.util
import functools

import numpy as np

import oracle as o

SENSITIVITY = 5.0
U23, U24 = 2.0 ** -23, 2.0 ** -24
F64, F32, F16 = np.float64, np.float32, np.float16

A_ROPE_CPU, A_EXP_CPU, A_TANH_CPU, A_SLOPE_CPU = 1.2, 0.51, 2.2, 6.5
DEVICE_MARGIN = 2.0


def dev_consts():
    return dict(rope=DEVICE_MARGIN * A_ROPE_CPU, exp=DEVICE_MARGIN * A_EXP_CPU, tanh=DEVICE_MARGIN * A_TANH_CPU, slope=DEVICE_MARGIN * A_SLOPE_CPU)


def cpu_consts():
    return dict(rope=A_ROPE_CPU, exp=A_EXP_CPU, tanh=A_TANH_CPU, slope=A_SLOPE_CPU)


def ulp16(v):
    """spacing of F16 at |v| (2^-24 below the normal range)"""
    a = np.abs(np.asarray(v, F64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15.0) - 10.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def half_dist(a, b):
    def key(v):
        u = bits(v).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(key(a) - key(b))


def within(got, ref, tol, what):
    """|got - ref| <= tol everywhere (NaN / inf in got where ref is finite fails); returns the worst err / tol"""
    g = np.asarray(got).astype(F64)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref)
    err = np.where(np.isnan(err), np.inf, err)
    ratio = err / tol
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: |got - f64| = %.3g > bound %.3g at %s (%.2f x)" % (what, err[i], np.broadcast_to(tol, err.shape)[i], i, worst))
    return worst


# ------------------------------------------------------------------ libm in fp32 (what the oracle's C code calls)
@functools.lru_cache(None)
def _libm():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for n in ("cosf", "sinf", "expf", "tanhf"):
        getattr(m, n).restype = C.c_float
        getattr(m, n).argtypes = [C.c_float]
    m.powf.restype = C.c_float
    m.powf.argtypes = [C.c_float, C.c_float]
    return m


# =================================================================== RoPE
class RopeCase:
    def __init__(self, hd, heads, tokens, pos0, theta=1e4, order=2, partial=1.0, table=None, seed=0):
        self.hd, self.heads, self.tokens, self.pos0, self.theta, self.order, self.partial = hd, heads, tokens, pos0, theta, order, partial
        self.rope_cols = int(hd * F32(partial) + F32(0.5))
        assert self.rope_cols % 2 == 0 and 0 < self.rope_cols <= hd
        self.pos = np.asarray(table, np.int64) if table is not None else pos0 + np.arange(tokens, dtype=np.int64)
        assert self.pos.size == tokens
        self.table = table is not None
        self.id = "hd%d-h%d-t%d-p%d-th%g-o%d-pr%g%s" % (hd, heads, tokens, int(self.pos[0]), theta, order, partial, "-tab" if self.table else "")
        rng = np.random.default_rng(1000 + seed + hd * 7 + heads * 131 + tokens)
        self.x = rng.normal(0, 1.0, (tokens, heads, hd)).astype(F16)
        self.ref, self.mag = rope_f64(self.x, self.pos, theta, order, self.rope_cols, self.rope_cols)

    def split(self):
        """rope_head_split of the wrapper: (y blocks, heads per block)"""
        pairs = self.tokens * (self.hd // 2)
        want = (32768 + pairs - 1) // pairs
        y = max(1, min(want, self.heads))
        return y, (self.heads + y - 1) // y

    def oracle(self):
        if not self.table:
            return o.rope(self.x, int(self.pos0), self.theta, self.order, self.partial)
        return np.concatenate([o.rope(self.x[t:t + 1], int(self.pos[t]), self.theta, self.order, self.partial) for t in range(self.tokens)])

    def tol(self, A):
        return rope_tol(self.ref, self.mag, self.pos, A)


def rope_f64(x, pos, theta, order, rope_cols, rope_dims, partner=None, heads=None):
    """x [T][H][hd] F16, pos [T]; float64 rotation of the written expression; returns (out, |x0| + |x1| per rotated element)"""
    T, H, hd = x.shape
    x64 = x.astype(F64)
    out, mag = x64.copy(), np.zeros(x64.shape)
    npairs = hd // 2 if order == 1 else rope_cols // 2
    col = np.arange(npairs)
    ts = float(F32(theta)) ** (-2.0 / rope_dims)
    ang = np.asarray(pos, F64)[:, None] * ts ** col[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    i0, i1 = (col, col + (partner if partner is not None else rope_cols // 2)) if order == 2 else (2 * col, 2 * col + 1)
    hs = slice(None) if heads is None else heads
    x0, x1 = x64[:, hs][:, :, i0], x64[:, hs][:, :, i1]
    o0, o1 = x0 * c - x1 * s, x0 * s + x1 * c
    sub, msub = out[:, hs], mag[:, hs]
    sub[:, :, i0], sub[:, :, i1] = o0, o1
    msub[:, :, i0] = msub[:, :, i1] = np.abs(x0) + np.abs(x1)
    out[:, hs], mag[:, hs] = sub, msub
    return out, mag


def rope_tol(ref, mag, pos, A):
    """two products and a sum in fp32 (<= 3 x 2^-24 of |x0| + |x1|), the angle and cosf / sinf (A x pos x 2^-23), one F16 rounding"""
    rest = mag * (3 * U24 + A * U23 * np.asarray(pos, F64)[:, None, None])
    return 0.5 * ulp16(np.abs(ref) + rest) + rest


def check_rope(got, c, A, what="rope"):
    """within the bound of float64; the elements no pair touches, and every element at position 0, keep their bits"""
    worst = within(got, c.ref, c.tol(A), what + " " + c.id)
    keep = (c.mag == 0) | (c.pos == 0)[:, None, None]
    assert np.array_equal(bits(got)[keep], bits(c.x)[keep]), what + " " + c.id + ": an element outside the rotation (or at position 0) changed"
    return worst


@functools.lru_cache(None)
def measure_rope(keys):
    """keys: tuple of (theta, rope_dims, npairs, positions tuple): libm's fp32 angle, cosf, sinf against float64, in pos x 2^-23"""
    m, worst = _libm(), 0.0
    for theta, rd, npairs, poss in keys:
        ts = m.powf(F32(theta), float(F32(-2.0) / F32(rd)))
        ts64 = float(F32(theta)) ** (-2.0 / rd)
        pw = [1.0] + [m.powf(ts, float(col)) for col in range(1, npairs)]
        for pos in poss:
            if pos == 0:
                continue
            for col in range(npairs):
                ang = float(F32(pos)) if col == 0 else float(F32(F32(pos) * F32(pw[col])))
                a64 = pos * ts64 ** col
                e = max(abs(m.cosf(ang) - np.cos(a64)), abs(m.sinf(ang) - np.sin(a64)))
                worst = max(worst, e / (pos * U23))
    return worst


def rope_measure_keys(cases):
    d = {}
    for c in cases:
        k = (c.theta, c.rope_cols, c.hd // 2 if c.order == 1 else c.rope_cols // 2)
        d.setdefault(k, set()).update(int(p) for p in c.pos)
    return tuple(sorted((k[0], k[1], k[2], tuple(sorted(v))) for k, v in d.items()))


def rope_cases():
    R = RopeCase
    cs = []
    # the block edges of k_rope: tokens * head_dim / 2 = 1, 255, 256, 257 threads; heads 1, 5, 32, 33
    cs += [R(2, 1, 1, 57), R(34, 5, 15, 0), R(32, 32, 16, 1), R(2, 33, 257, 4095 - 256), R(514, 5, 1, 32767)]
    # every head_dim x order x partial rotary, theta 1e4 / 1e6, positions 0, 1, 57, 4095, 32767 in turn
    poss = [0, 1, 57, 4095 - 2, 32767 - 2]
    i = 0
    for hd in (32, 64, 80, 128, 256):
        for order in (1, 2):
            for partial in (1.0, 0.5, 0.25):
                cs.append(R(hd, (1, 5, 3)[i % 3], 3, poss[i % 5], (1e4, 1e6)[(i // 2) % 2], order, partial, seed=i))
                i += 1
    cs.append(R(128, 4, 3, 57, 1e4, 2, 1.0, seed=91))                 # the shape of tests/test_gpu_ops.py::test_rope
    cs.append(R(256, 2, 256, 32767 - 255, 1e6, 2, 0.5, seed=92))      # 32768 pairs: a head split of 1
    cs.append(R(128, 5, 128, 4095 - 127, 1e4, 1, 1.0, seed=93))       # split 4 over 5 heads: 2 + 2 + 1 + none
    assert cs[-2].split() == (1, 2) and cs[-1].split() == (4, 2)
    return cs


ROWS_TABLE = [57, 0, 4095, 57, 3, 0, 32767, 1]      # non-monotonic, repeats, zeros


def rope_rows_cases():
    return [RopeCase(hd, heads, len(ROWS_TABLE), 0, theta, order, partial, table=ROWS_TABLE, seed=50 + hd)
            for hd, heads, theta, order, partial in [(64, 5, 1e4, 2, 1.0), (128, 2, 1e6, 1, 0.5), (80, 3, 1e4, 2, 0.5), (32, 33, 1e6, 1, 1.0)]]


def rope_faults(c):
    """(name, float64 output carrying the fault) for the faults this case can show"""
    x, pos, th, od, rc = c.x, c.pos, c.theta, c.order, c.rope_cols
    out = []
    if od == 2 and rc < c.hd:
        out.append(("partner column col + head_dim / 2", rope_f64(x, pos, th, od, rc, rc, partner=c.hd // 2)[0]))
        tail = rope_f64(np.ascontiguousarray(x[:, :, rc:]), pos, th, 2, c.hd - rc, rc)[0] if (c.hd - rc) % 2 == 0 else None
        if tail is not None:
            f = c.ref.copy()
            f[:, :, rc:] = tail
            out.append(("the unrotated tail rotated", f))
    if rc < c.hd:
        out.append(("rope_dims = head_dim under partial rotary", rope_f64(x, pos, th, od, rc, c.hd)[0]))
    if rc == c.hd or od == 1:
        out.append(("order 1 and 2 exchanged", rope_f64(x, pos, th, 3 - od, rc if od == 1 else c.hd, rc)[0]))
    out.append(("position off by one", rope_f64(x, pos + 1, th, od, rc, rc)[0]))
    if c.table:
        out.append(("pos0 + t in place of the table's position", rope_f64(x, pos[0] + np.arange(c.tokens), th, od, rc, rc)[0]))
    y, hpb = c.split()
    if c.heads > 1:
        last = min(c.heads, hpb) - 1           # the last head of the first y block
        f = c.ref.copy()
        f[:, last] = x[:, last].astype(F64)
        out.append(("the last head of a split skipped", f))
        twice = rope_f64(c.ref.astype(F16), pos, th, od, rc, rc, heads=[last])[0]
        g = c.ref.copy()
        g[:, last] = twice[:, last]
        out.append(("a head rotated twice", g))
    return out


def carry(orc, ref, faulty):
    """the oracle's output with the fault applied: the elements the fault moves take its (F16-rounded) values"""
    bad = orc.copy()
    moved = faulty != ref
    bad[moved] = faulty.astype(F16)[moved]
    return bad


# ----- the fused q / k / cache launch
class StoreCase:
    def __init__(self, hd, heads, kv_heads, tokens=3, pos0=5, theta=1e4, order=2, partial=1.0, caches=True, gap=0, seed=0):
        self.hd, self.heads, self.kv_heads, self.tokens, self.pos0 = hd, heads, kv_heads, tokens, pos0
        self.theta, self.order, self.partial, self.caches, self.gap = theta, order, partial, caches, gap
        self.kv_dim = kv_heads * hd
        self.row_elems = self.kv_dim + gap
        self.q = RopeCase(hd, heads, tokens, pos0, theta, order, partial, seed=seed)
        self.k = RopeCase(hd, kv_heads, tokens, pos0, theta, order, partial, seed=seed + 1)
        self.v = np.random.default_rng(seed + 77).normal(0, 1.0, (tokens, self.kv_dim)).astype(F16)
        self.cache_rows = pos0 + tokens + 2
        self.vector = self.q.rope_cols == hd and hd % 16 == 0
        self.id = "hd%d-h%d-kv%d-o%d-pr%g-%s-gap%d" % (hd, heads, kv_heads, order, partial, "f16" if caches else "null", gap)

    def sentinel_cache(self):
        return np.full((self.cache_rows, self.row_elems), 0xABCD, np.uint16)

    def expected_cache(self, rows):
        """rows [tokens][kv_dim] (bit patterns): the cache with those rows at pos0 .. pos0 + tokens - 1, everything else the sentinel"""
        e = self.sentinel_cache()
        e[self.pos0:self.pos0 + self.tokens, :self.kv_dim] = bits(rows).reshape(self.tokens, self.kv_dim)
        return e


def store_cases():
    S = StoreCase
    return [
        S(64, 4, 4, seed=1), S(128, 8, 2, order=1, gap=24, seed=2), S(256, 4, 1, theta=1e6, seed=3),          # MHA, GQA 4, one KV head
        S(48, 85, 5, tokens=2, seed=4), S(128, 32, 8, tokens=2, order=1, seed=5), S(16, 257, 257, tokens=2, caches=False, seed=6),   # 255 / 256 / 257 items
        S(8, 1, 1, seed=7), S(128, 16, 16, tokens=2, gap=8, seed=8), S(128, 17, 17, tokens=2, seed=9),        # kv_dim 8, 2048, 2176
        S(80, 5, 5, order=2, seed=10), S(80, 4, 1, order=1, caches=False, seed=11),                            # head_dim 80: vector path (80 % 16 == 0)
        S(72, 4, 2, seed=12), S(72, 3, 3, order=1, seed=13),                                                   # head_dim % 16 == 8: scalar path
        S(64, 8, 2, partial=0.5, seed=14), S(128, 4, 4, order=1, partial=0.25, caches=False, seed=15), S(32, 4, 1, partial=0.5, gap=8, theta=1e6, seed=16),
    ]


def check_store(c, q, k, v, kc, vc, A, q_rope=None, k_rope=None):
    """q, k [tokens][heads][hd] after the launch, v after it, kc / vc the whole cache buffers (uint16) or None;
    q_rope / k_rope: what ifa_rope left on the same inputs (device test) -- must be the same bits"""
    worst = max(check_rope(q, c.q, A, "qk_store q"), check_rope(k, c.k, A, "qk_store k"))
    assert same_bits(v, c.v), c.id + ": v changed"
    if q_rope is not None:
        assert same_bits(q, q_rope) and same_bits(k, k_rope), c.id + ": q / k differ from ifa_rope on the same inputs"
    if c.caches:
        assert np.array_equal(kc, c.expected_cache(k)), c.id + ": k cache rows are not the rotated k rows, or bytes outside them changed"
        assert np.array_equal(vc, c.expected_cache(c.v)), c.id + ": v cache rows are not v, or bytes outside them changed"
    return worst


def store_cache_faults(c, k_rot):
    """(name, kcache, vcache) for F16-cache cases"""
    good_k, good_v = c.expected_cache(k_rot), c.expected_cache(c.v)
    late = c.sentinel_cache()
    late[c.pos0 + 1:c.pos0 + 1 + c.tokens, :c.kv_dim] = bits(k_rot).reshape(c.tokens, c.kv_dim)
    out = [("the k cache row one position late", late, good_v), ("v written to the k cache", good_v, good_v)]
    if c.gap:
        g = good_k.copy()
        g[c.pos0, c.kv_dim] = 0
        out.append(("the stride gap written", g, good_v))
    return out


# (args of ifa_rope_qk_store as a dict, why) -- each refusal next to the accepted call it was made from
def store_refusals():
    base = dict(q=0x10000, k=0x20000, v=0x30000, hd=64, heads=4, kv_heads=2, tokens=2, pos0=0, theta=1e4, order=2, partial=1.0,
                kc=0x40000, vc=0x50000, row_elems=128)
    r = [("order 0", dict(order=0)), ("order 3", dict(order=3)), ("odd head_dim", dict(hd=63, kv_heads=8)), ("kv_dim % 8", dict(hd=6, kv_heads=2, row_elems=16)),
         ("vcache without v", dict(v=0)), ("cache_row_elems % 8", dict(row_elems=132)), ("LDS beyond 64 KiB", dict(hd=128, kv_heads=255, heads=255, row_elems=128 * 255))]
    for name in ("q", "k", "v", "kc", "vc"):
        r.append(("misaligned " + name, {name: base[name] + 2}))
    return base, [(why, dict(base, **d)) for why, d in r]


# =================================================================== norms
NORM_COLS = [1, 7, 8, 9, 127, 128, 129, 511, 512, 513, 520, 1001, 4097]
NORM_FORMS = ["w", "wb", "none", "w+1"]


def norm_inputs(cols, rows=3, seed=0):
    """two row sets: A = outlier of 30 in the LAST column / constant / all-zero, B = magnitudes near 65504 / 8 / normal / normal"""
    rng = np.random.default_rng(31 * cols + seed)
    a = rng.normal(0, 1.0, (3, cols))
    a[0, cols - 1] = 30.0
    a[1, :] = 0.125
    a[2, :] = 0.0
    b = rng.normal(0.3, 1.0, (3, cols))
    b[0] = rng.uniform(0.5, 1.0, cols) * 8188.0 * rng.choice([-1.0, 1.0], cols)
    w = rng.normal(1, 0.1, cols).astype(F16)
    bias = rng.normal(0, 0.1, cols).astype(F16)
    return a[:rows].astype(F16), b[:rows].astype(F16), w, bias


def form_args(form, w, b):
    return {"w": (w, None, 0.0), "wb": (w, b, 0.0), "none": (None, None, 0.0), "w+1": (w, None, 1.0)}[form]


def rms_f64(x, w, b, mb, eps=1e-5, drop_from=None, mean_cols=None):
    x64 = x.astype(F64)
    xs = x64 if drop_from is None else x64[:, :drop_from]
    t = x64 / np.sqrt((xs * xs).sum(1, keepdims=True) / (mean_cols or x.shape[1]) + eps)
    mag = np.abs(t)
    if w is not None:
        t = t * (mb + w.astype(F64))
        mag = np.abs(t)
        if b is not None:
            t = t + b.astype(F64)
            mag = mag + np.abs(b.astype(F64))
    return t, mag


def std_f64(x, w, b, eps=1e-5):
    """float64 std norm and its bound: the fp32 sums (33 strided terms and 128 partials at 4097 columns: relative error
    <= delta = (ceil(cols / 128) + 128) x 2^-24 of the sum of magnitudes) move the mean by dm and the variance by dv"""
    x64 = x.astype(F64)
    cols = x.shape[1]
    mean = x64.mean(1, keepdims=True)
    ex2 = (x64 * x64).mean(1, keepdims=True)
    var = ex2 - mean * mean
    scale = 1.0 / np.sqrt(var + eps)
    t = (x64 - mean) * scale
    delta = ((cols + 127) // 128 + 128 + 4) * U24
    dm = delta * np.abs(x64).mean(1, keepdims=True)
    dv = delta * ex2 + 2 * np.abs(mean) * dm + dm * dm
    err = dm * scale + np.abs(x64 - mean) * scale * 0.5 * dv / (var + eps)
    mag = np.abs(t)
    if w is not None:
        wm = np.abs(w.astype(F64))
        t, err, mag = t * w.astype(F64), err * wm, mag * wm
        if b is not None:
            t = t + b.astype(F64)
            mag = mag + np.abs(b.astype(F64))
    return t, err + 6 * U24 * mag


def check_norm(kind, got, x, w, b, mb, what):
    """tests/test_gpu_ops.py's bounds: RMS within one half ulp of the oracle, >= 99.5 % identical, inside its float64 expression;
    std norm bit-exact with the oracle (and inside float64)"""
    if kind == 0:
        exp = o.rmsnorm(x, w, b, multi_base=mb)
        d = half_dist(got, exp)
        assert d.max() <= 1 and (d == 0).mean() >= 0.995, "%s: %d half ulps from the oracle, %.2f %% identical" % (what, int(d.max()), 100 * float((d == 0).mean()))
        t, mag = rms_f64(x, w, b, mb)
        u = np.spacing(np.abs(got).astype(F16)).astype(F64)
        return within(got, t, 0.501 * np.maximum(u, U24) + 4 * U24 * mag, what)
    assert same_bits(got, o.stdnorm(x, w, b)), what + ": not the oracle's bits"
    t, extra = std_f64(x, w, b)
    return within(got, t, 0.501 * ulp16(np.abs(t) + extra) + extra, what)


def check_add_norm(kind, sum_out, y, a, addend, w, b, mb, what):
    assert same_bits(sum_out, o.add(a, addend)), what + ": sum_out is not the half-rounded a + addend"
    return check_norm(kind, y, np.ascontiguousarray(sum_out), w, b, mb, what)


def norm_faults(kind, x, w, b, mb):
    """(name, faulty F16 output) -- applied to the oracle's output through `carry`"""
    cols = x.shape[1]
    out = []

    def model(xx=x, ww=w, bb=b, m=mb, **kw):
        return (rms_f64(xx, ww, bb, m, **kw) if kind == 0 else std_f64(xx, ww, bb))[0]
    if kind == 0:
        if cols % 8 and cols > 8:
            out.append(("the last cols % 8 elements left out of the sum", model(drop_from=cols - cols % 8)))
        ngroups = ((cols + 7) // 8 + 63) // 64
        if ngroups > 1:
            out.append(("the last group left out", model(drop_from=512 * (ngroups - 1))))
        if cols % 8:
            out.append(("cols rounded up in the mean", model(mean_cols=(cols + 7) // 8 * 8)))
        if w is not None and mb != 0.0:
            out.append(("multi_base dropped", model(m=0.0)))
    if cols > 1 and w is not None:
        out.append(("weight of the neighbouring column", model(ww=np.roll(w, 1))))
        if b is not None:
            out.append(("bias of the neighbouring column", model(bb=np.roll(b, 1))))
    return out


# =================================================================== activation
def all_finite_halves():
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = u.view(F16)
    return h[np.isfinite(h)].copy()


def act_f64(v, kind):
    """float64 activation and the fp32 terms of its bound (without the final F16 rounding)"""
    v = np.asarray(v).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == 0:
            e = np.exp(-v)
            f = np.where(np.isinf(e), -0.0, v / (1.0 + e))
            return f, np.abs(f) * U23, np.abs(f) * U23 * np.where(np.isinf(e), 0.0, e / (1.0 + e))       # add + divide; expf's ulps reach f through e / (1 + e)
        if kind == 1:
            a = 0.79788456080286535587989211986876 * v * (1.0 + 0.044715 * v * v)
            th = np.tanh(a)
            f = 0.5 * v * (1.0 + th)
            # v2, inner, a (twice), 1 + t, 0.5 v t: <= 3 x 2^-23 relative of f besides tanhf; an argument error da moves tanh by (1 - th^2) da
            arg = np.abs(a) * 4 * U24 * (1.0 - th * th)
            return f, np.abs(f) * 3 * U23 + 0.5 * np.abs(v) * arg, 0.5 * np.abs(v) * np.abs(th) * U23
        return np.maximum(v, 0.0), np.zeros(v.shape), np.zeros(v.shape)


def act_tol(v, kind, k):
    f, fixed, per_ulp = act_f64(v, kind)
    rest = fixed + per_ulp * (k["exp"] if kind == 0 else k["tanh"])
    return f, 0.5 * ulp16(np.abs(f) + rest) + rest


def check_act(got, v, kind, k, what):
    f, tol = act_tol(v, kind, k)
    return within(got, f, tol, what)


def glu_f64(x, kind, k):
    """x [rows][2 cols]: act(x[:, :cols]) * x[:, cols:], one F16 rounding (the product is taken in fp32)"""
    cols = x.shape[1] // 2
    f, fixed, per_ulp = act_f64(x[:, :cols], kind)
    g = x[:, cols:].astype(F64)
    rest = (fixed + per_ulp * (k["exp"] if kind == 0 else k["tanh"])) * np.abs(g) + np.abs(f * g) * U24
    return f * g, 0.5 * ulp16(np.abs(f * g) + rest) + rest


def act_mul_f64(a, b, kind, k):
    """c = half(half(act(a)) * b): the activation's bound times |b|, and the product's rounding"""
    f, tol = act_tol(a, kind, k)
    b64 = np.asarray(b).astype(F64)
    ref = f.astype(F16).astype(F64) * b64
    rest = np.abs(b64) * (tol + 0.5 * ulp16(f))
    return ref, 0.5 * ulp16(np.abs(ref) + rest) + rest


def check_act_mul(got, a, b, kind, k, what, dev_act=None):
    """bit-identical to o.mul(o.act(a), b) wherever the activation launch (dev_act; the oracle itself on the host) equals the oracle"""
    oa = o.act(a.reshape(1, -1), kind).reshape(a.shape)
    same = np.ones(a.shape, bool) if dev_act is None else bits(dev_act) == bits(oa)
    exp = o.mul(oa, b)
    # the identity must not become vacuous: the two activations differ where a device expf / tanhf ulp flips an F16 rounding, rarely
    assert (~same).sum() <= max(1, 0.01 * same.size), "%s: the activation launch equals the oracle on %.1f %% of the elements only" % (what, 100 * same.mean())
    assert np.array_equal(bits(got)[same], bits(exp)[same]), what + ": not o.mul(o.act(a), b) where the activation agrees with the oracle"
    ref, tol = act_mul_f64(a, b, kind, k)
    fin = np.isfinite(ref)
    return within(np.asarray(got)[fin], ref[fin], tol[fin], what)


ACT_MUL_N = [8, 2048, 2056, 7, 2049]


def act_mul_inputs(n, seed=0):
    rng = np.random.default_rng(900 + n + seed)
    a = rng.normal(0, 2.0, n).astype(F16)
    b = rng.normal(0, 2.0, n).astype(F16)
    b[: n // 3] = 0.0
    b[n // 3: n // 2] = 1.0
    return a, b


def act_mul_faults(a, b, kind):
    with np.errstate(over="ignore", invalid="ignore"):
        f = act_f64(a, kind)[0]
        g = [("the intermediate half rounding dropped", (f.astype(F32) * b.astype(F32)).astype(F16)),
             ("the multiplier of the neighbouring element", (f.astype(F16).astype(F32) * np.roll(b, 1).astype(F32)).astype(F16)),
             ("the kind ignored", (act_f64(a, (kind + 1) % 3)[0].astype(F16).astype(F32) * b.astype(F32)).astype(F16))]
    return g


@functools.lru_cache(None)
def measure_act():
    """libm's expf(-v) and tanhf(a) against float64 over every finite half, in fp32 ulps of the result"""
    m = _libm()
    we = wt = 0.0
    for v in all_finite_halves().astype(F64):
        e32, e64 = m.expf(-v), np.exp(-v) if -v < 700 else np.inf
        if np.isfinite(e32) and 2.0 ** -126 < e64 < 3e38:
            we = max(we, abs(e32 - e64) / float(np.spacing(F32(e64))))
        v32 = F32(v)
        a = F32(F32(F32(0.79788456080286535587989211986876) * v32) * F32(F32(1.0) + F32(F32(0.044715) * F32(v32 * v32))))
        if np.isfinite(a) and abs(float(a)) > 2.0 ** -100:
            t64 = np.tanh(float(a))
            wt = max(wt, abs(m.tanhf(float(a)) - t64) / float(np.spacing(F32(t64))))
    return we, wt


# =================================================================== argmax
def argmax_ref(v, excl=()):
    """first maximum among the ids that are not excluded and not NaN; 0 when there is none"""
    f = np.asarray(v).astype(F32)
    ok = ~np.isnan(f)
    for e in excl:
        if 0 <= e < f.size:
            ok[e] = False
    if not ok.any():
        return 0
    m = f[ok].max()
    return int(np.flatnonzero(ok & (f == m))[0])


def excl_words(ids, count=None):
    """the {count, id, id, id} block of the launch and the ids that count (count clamped to 0 .. 3)"""
    w = np.full(4, -1, np.int32)
    w[1:1 + len(ids)] = ids
    w[0] = len(ids) if count is None else count
    return w, [int(i) for i in w[1:1 + min(max(int(w[0]), 0), 3)]]


ARGMAX_N = [1, 3, 7, 8, 9, 32767, 32768, 32776, 40001]


def argmax_vectors(n):
    """(name, vector, exclusion words or None) for one length"""
    rng = np.random.default_rng(n)
    base = rng.normal(0, 1.0, n).astype(F16)
    base = np.minimum(base, F16(3.0))
    out = [("random", base, None)]

    def with_max(ids, val=5.0, b=base):
        v = b.copy()
        v[[i for i in ids if i < n]] = val
        return v
    ties = {"same chunk": (17, 19), "across threads": (8 * 5 + 1, 8 * 700 + 1), "across slots": (8 * 3 + 2, 8 * (1024 + 3) + 2, 8 * (3072 + 3) + 2),
            "across waves": (8 * 67 + 4, 8 * 3 + 4), "vector and tail": (100, n - 1), "tail only": (n - 1,), "last chunk": (max(0, (n // 8) * 8 - 3),)}
    for name, ids in ties.items():
        if max(ids) < n or name in ("vector and tail",):
            out.append(("max " + name, with_max(ids), None))
    out.append(("all equal", np.full(n, 0.5, F16), None))
    out.append(("all -inf", np.full(n, -np.inf, F16), None))
    out.append(("all NaN", np.full(n, np.nan, F16), None))
    v = with_max((n // 2,))
    v[::3] = np.nan
    v[n // 2] = 5.0
    out.append(("NaNs present", v, None))
    for cnt, ids in [(0, [n - 1]), (1, [n - 1]), (2, [n - 1, 0]), (3, [n - 1, 0, n // 2]), (5, [n - 1, 0, n // 2]), (-1, [n - 1])]:
        out.append(("excl count %d, maximum excluded in the tail" % cnt, with_max((n - 1, 0)), excl_words(ids, cnt)[0]))
    last_chunk_id = max(0, (n // 8) * 8 - 3)
    out.append(("maximum excluded in the last chunk", with_max((last_chunk_id,)), excl_words([last_chunk_id])[0]))
    out.append(("maximum excluded at id 0", with_max((0,)), excl_words([0])[0]))
    if n == 3:          # e0, e1, e2 together leave no candidate, neither in a chunk nor in the tail: the result is 0
        out.append(("every id excluded", np.array([1.0, 3.0, 2.0], F16), excl_words([0, 1, 2])[0]))
        out.append(("every id excluded, maximum first", np.array([3.0, 1.0, 2.0], F16), excl_words([2, 0, 1])[0]))
    return out


def excluded_of(words):
    return [] if words is None else [int(i) for i in words[1:1 + min(max(int(words[0]), 0), 3)]]


def argmax_faults(v, words, aligned=True, nthreads=1024):
    """(name, the id a kernel with the fault would return)"""
    f = np.asarray(v).astype(F32)
    n, ex = f.size, excluded_of(words)
    ok = ~np.isnan(f)
    for e in ex:
        if 0 <= e < n:
            ok[e] = False
    chunks = n // 8 if aligned else 0
    out = []
    if ok.any():
        out.append(("last maximum wins", int(np.flatnonzero(ok & (f == f[ok].max()))[-1])))
    out.append(("the tail ignored", argmax_ref(v[:chunks * 8], ex) if chunks else 0))
    out.append(("the exclusion ignored", argmax_ref(v, ())))
    # the clamped slot counted: a thread whose slot lies past the last chunk reads the last chunk and reports ids past n
    if chunks:
        steps = (chunks + 4 * nthreads - 1) // (4 * nthreads)
        first_phantom = chunks                      # the lowest slot index >= chunks that some thread visits
        if first_phantom < steps * 4 * nthreads:
            ids = first_phantom * 8 + np.arange(8)
            vals = f[(chunks - 1) * 8: chunks * 8]
            okp = ~np.isnan(vals) & ~np.isin(ids, ex)
            true = argmax_ref(v, ex)
            best = f[true] if ok.any() else -np.inf
            if okp.any() and (vals[okp].max() > best or not ok.any()):
                out.append(("the clamped slot counted", int(ids[okp][np.argmax(vals[okp])])))
            else:
                out.append(("the clamped slot counted", true))
    return out


# =================================================================== ALiBi
def alibi_slopes64(total_heads):
    hl2 = 1 << int(np.floor(np.log2(total_heads)))
    h = np.arange(total_heads)
    return np.where(h < hl2, 2.0 ** (-8.0 * (h + 1) / hl2), 2.0 ** (-4.0 * (2 * (h - hl2) + 1) / hl2)), hl2


class AlibiCase:
    def __init__(self, heads, qt, ctx, base, total, seed=0):
        self.heads, self.qt, self.ctx, self.base, self.total = heads, qt, ctx, base, total
        self.id = "h%d-q%d-c%d-b%d-of%d" % (heads, qt, ctx, base, total)
        self.s = np.random.default_rng(seed + heads * ctx).normal(0, 0.5, (heads, qt, ctx)).astype(F16)
        self.ref, self.bias = self.model(lambda h, q: h + base)

    def model(self, head_of, first_family_only=False):
        sl, hl2 = alibi_slopes64(self.total)
        if first_family_only:
            sl = 2.0 ** (-8.0 * (np.arange(self.total) + 1) / hl2)
        h = np.arange(self.heads)[:, None, None]
        q = np.arange(self.qt)[None, :, None]
        idx = np.broadcast_to(head_of(h, q), (self.heads, self.qt, 1)) % self.total
        bias = np.arange(self.ctx)[None, None, :] * sl[idx]
        return bias + self.s.astype(F64), bias

    def tol(self, k):
        rest = np.abs(self.bias) * (U24 + k["slope"] * U23) + np.abs(self.ref) * U24
        return 0.5 * ulp16(np.abs(self.ref) + rest) + rest

    def faults(self):
        out = []
        if self.base:
            out.append(("the slope of h in place of h + base_head", self.model(lambda h, q: h)[0]))
        hl2 = alibi_slopes64(self.total)[1]
        if self.base + self.heads > hl2:
            out.append(("the first family past hl2", self.model(lambda h, q: h + self.base, first_family_only=True)[0]))
        if self.qt > 1:
            out.append(("the slope indexed by the query row", self.model(lambda h, q: q + self.base + 0 * h)[0]))
        return out


def alibi_cases():
    A = AlibiCase
    return [A(5, 3, 17, 0, 8, 1), A(8, 2, 16, 0, 8, 2), A(1, 1, 257, 11, 12, 3), A(6, 2, 100, 6, 12, 4), A(16, 3, 40, 0, 16, 5),
            A(8, 2, 300, 8, 16, 6), A(10, 2, 64, 30, 40, 7), A(40, 1, 33, 0, 40, 8)]


@functools.lru_cache(None)
def measure_slope():
    m, worst = _libm(), 0.0
    for total in (8, 12, 16, 40):
        s64, hl2 = alibi_slopes64(total)
        m0, m1 = m.powf(2.0, float(F32(-8.0) / F32(hl2))), m.powf(2.0, float(F32(-4.0) / F32(hl2)))
        for h in range(total):
            mk = m.powf(m0, float(h + 1)) if h < hl2 else m.powf(m1, float(2 * (h - hl2) + 1))
            worst = max(worst, abs(mk - s64[h]) / float(np.spacing(F32(s64[h]))))
    return worst


# =================================================================== softmax
class SoftmaxCase:
    def __init__(self, cx, cy, cz, prefix, scale, seed=0, plant=True):
        self.cx, self.cy, self.cz, self.prefix, self.scale = cx, cy, cz, prefix, scale
        self.id = "cx%d-cy%d-cz%d-p%d-s%g" % (cx, cy, cz, prefix, scale)
        rng = np.random.default_rng(seed + cx)
        s = rng.normal(0, 2.0, (cz, cy, cx)).astype(F16)
        if plant:
            s[0, 0, 0] = 65504.0             # a row holding the largest half
        if plant and cy > 1:
            s[0, 1, :] = 1.5                 # a row of equal values
        self.s = s
        v = float(F32(scale)) * s.astype(F64)
        self.masked = np.zeros(s.shape, bool)
        if prefix >= 0:
            self.masked = np.arange(cx)[None, None, :] > prefix + np.arange(cy)[None, :, None]
            self.masked = np.broadcast_to(self.masked, s.shape)
        v = np.where(self.masked, -np.inf, v)
        mx = v.max(-1, keepdims=True)
        e = np.exp(v - mx)
        self.ref = e / e.sum(-1, keepdims=True)
        self.arg = np.where(self.masked, 0.0, np.abs(np.where(self.masked, 0.0, v)) + np.abs(mx))

    def tol(self, k):
        """e and e / sum are rounded to F16 (2^-11 each, and the sum of rounded e's moves by 2^-11 at most); expf's ulps; the fp32
        roundings of scale * s and of v - max scale with the arguments; the fp32 sum of <= 10 terms a lane and 5 butterfly steps"""
        rel = 3 * 2.0 ** -11 + (k["exp"] + 16) * U23 + 2 * U24 * self.arg
        return self.ref * rel + 2 * 2.0 ** -25


def softmax_cases():
    S = SoftmaxCase
    return [S(1, 3, 1, -1, 1.0), S(31, 3, 1, 0, 1.0), S(32, 2, 2, -1, 0.125), S(33, 5, 1, 40, 1.0), S(77, 3, 2, 40, 1.5), S(300, 3, 1, 40, 0.125),
            S(300, 1, 1, -1, 1.0), S(77, 5, 1, 0, 0.125)]


def check_softmax(got, c, k):
    worst = within(got, c.ref, c.tol(k), "softmax " + c.id)
    assert (bits(got)[c.masked] == 0).all(), "softmax " + c.id + ": the masked tail is not exactly 0"
    return worst


# =================================================================== record of the worst err / bound per launch (printed by the device test)
WORST = {}


def note(launch, ratio):
    WORST[launch] = max(WORST.get(launch, 0.0), float(ratio))
    return ratio
