"""Reference, inputs and assertions of the decode-attention edge tests (tests/test_decode_attn_ref_cpu.py on the host,
tests/test_gpu_decode_attn_edges.py on the device).

The single-query decode attention is  out[h] = softmax_j(q[h] . K[j, kv(h)] / sqrt(head_dim) [+ j * slope(h)]) . V[j, kv(h)]  over the
n = p + 1 rows of the cache, row p being the step's own key / value.  Three things live here:

  * ref_attention_f64 / ref_rope_f64: that formula in numpy float64 with NO intermediate rounding, on the cache rows as the device
    holds them (F16 values, or Q8_B32T2 blocks dequantised exactly as scale x code).  ALiBi slopes and the query-head -> kv-head map are
    written from the reference's definition (PosEmbedding_Alibi_Std_Kernel; head h reads kv head h / (heads / kv_heads)).
  * input families (dense / flat / needle) and key mutations (delete / duplicate / swap with the neighbour / wrong kv head), with the
    sensitivity condition: a mutation of one probed key moves the float64 output by >= 5 x the float64 tolerance of the case.
  * the assertions the GPU test applies to the device's output (check_att, check_new_row, check_attq), as functions, so that the CPU
    test can feed them MUTATED oracle outputs and see every one rejected.

Tolerances:
  att against oracle.attention:  6e-3 x max(1, max|V|)                      (the bound of test_attention in tests/test_gpu_ops.py)
  att against float64:           max(2 x d_ref, one F16 ulp at max|out|)     d_ref = max|oracle.attention - float64| of the SAME case:
                                 the distance of the reference's rounding points (S, e, P and O are F16) from exact math; the factor 2
                                 leaves room for the device's expf and another order of the fp32 sums on top of that.
The sensitivity condition is stated against the float64 tolerance (the tight one of the two)."""
import numpy as np

import oracle as o
from inferflow_amd import dtypes as dt

BUCKETS = (64, 128, 256, 512)
SENSITIVITY = 5.0           # a mutation of one probed key moves the float64 output by >= SENSITIVITY x tolerance
NEEDLE_WEIGHT = 0.9
FLAT_SCORE = 0.1


# ----------------------------------------------------------------------------- small helpers
def ulp16(x):
    """one F16 ulp at magnitude |x| (numpy array or scalar), subnormal spacing below 2^-14"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def kv_row_bytes(kv_dtype, kv_dim):
    return kv_dim * 2 if kv_dtype == dt.F16 else kv_dim // 32 * 34


def rows_f64(rows, kv_dtype, kv_dim):
    """cache rows as the device holds them -> float64 [n][kv_dim]; Q8_B32T2 blocks (F16 scale, 32 int8 codes) exactly as scale x code"""
    if kv_dtype == dt.F16:
        return np.ascontiguousarray(rows).view(np.float16).reshape(-1, kv_dim).astype(np.float64)
    b = np.ascontiguousarray(rows, np.uint8).reshape(-1, kv_dim // 32, 34)
    scale = b[:, :, :2].copy().view(np.float16).astype(np.float64)          # [n][blocks][1]
    codes = b[:, :, 2:].view(np.int8).astype(np.float64)                    # [n][blocks][32]
    return (codes * scale).reshape(-1, kv_dim)


def pack_rows(x16, kv_dtype):
    """F16 values [n][kv_dim] -> the bytes of n cache rows (uint8 [n][row bytes]) as the reference stores them"""
    x16 = np.ascontiguousarray(x16, np.float16)
    if kv_dtype == dt.F16:
        return x16.view(np.uint8).reshape(x16.shape[0], -1).copy()
    return o.quantize_act_q8(x16).reshape(x16.shape[0], -1)


def alibi_slopes(heads, base_head=0, total_heads=None):
    """slope of head h of a model with total_heads heads: with H2 = the largest power of two <= total_heads,
    2^(-8 / H2 * (h + 1)) for h < H2 and 2^(-4 / H2 * (2 (h - H2) + 1)) beyond; the bias of key j is j * slope"""
    total = total_heads or heads
    h2 = 1 << int(np.floor(np.log2(total)))
    idx = np.arange(heads, dtype=np.float64) + base_head
    return np.where(idx < h2, 2.0 ** (-8.0 / h2 * (idx + 1)), 2.0 ** (-4.0 / h2 * (2 * (idx - h2) + 1)))


def kv_head_of(heads, kv_heads, shift=0):
    """query head -> kv head: consecutive groups of heads / kv_heads query heads share one kv head (shift != 0: a WRONG map, for
    the mutation tests)"""
    return (np.arange(heads) // (heads // kv_heads) + shift) % kv_heads


# ----------------------------------------------------------------------------- float64 reference
def ref_rope_f64(x, pos, theta=10000.0, order=2, partial_rotary=1.0):
    """x: [heads][head_dim] (F16 values) at position pos -> float64, unrounded.  order 2: pairs (c, c + r / 2) of the first
    r = int(head_dim * partial_rotary + 0.5) columns; order 1: pairs (2 c, 2 c + 1) of the whole head; order 0: no rotation.
    Pair c turns by pos * theta^(-2 c / r)."""
    x = np.asarray(x).astype(np.float64)
    hd = x.shape[-1]
    r = int(hd * partial_rotary + 0.5)
    out = x.copy()
    if order == 0:
        return out
    if order == 2:
        c = np.arange(r // 2)
        i0, i1 = c, c + r // 2
    else:
        c = np.arange(hd // 2)
        i0, i1 = 2 * c, 2 * c + 1
    ang = float(pos) * np.power(float(theta), -2.0 * c / r)
    cs, sn = np.cos(ang), np.sin(ang)
    out[..., i0] = x[..., i0] * cs - x[..., i1] * sn
    out[..., i1] = x[..., i0] * sn + x[..., i1] * cs
    return out


def rope_tolerance(x, order=2, partial_rotary=1.0):
    """per element of x [heads][head_dim]: one F16 ulp at the length of the PAIR the element is rotated with (an unrotated element:
    its own size).  A rotation keeps the pair's length, not the element's: where the two products nearly cancel the result is small,
    but it still carries the error of the float32 angle pos * powf(powf(theta, -2 / r), c) -- (c + 3) float32 roundings, up to
    ~2.5e-4 rad at 700 positions -- times that length, next to half an ulp of its own rounding.  This is the bound of the oracle's
    rotation against float64 (measured 0.60) and of the device's small elements against the oracle's (check_new_row)."""
    x = np.asarray(x).astype(np.float64)
    hd = x.shape[-1]
    r = int(hd * partial_rotary + 0.5)
    mag = np.abs(x)
    if order == 2:
        c = np.arange(r // 2)
        i0, i1 = c, c + r // 2
    elif order != 0:
        c = np.arange(hd // 2)
        i0, i1 = 2 * c, 2 * c + 1
    if order != 0:
        norm = np.hypot(x[..., i0], x[..., i1])
        mag[..., i0] = norm
        mag[..., i1] = norm
    return ulp16(mag)


def ref_scores_f64(q_rot, k_rows, kv_dtype, heads, kv_heads, head_dim, kq_scale=1.0, use_alibi=False, alibi_base_head=0,
                   alibi_total_heads=None, head_shift=0):
    """float64 [heads][n]: q . K / sqrt(head_dim) (+ kq_scale * j * slope: the reference adds the bias to alpha * q.K with
    alpha = 1 / sqrt(head_dim) / kq_scale and its softmax multiplies by kq_scale)"""
    q = np.asarray(q_rot).astype(np.float64).reshape(heads, head_dim)
    K = rows_f64(k_rows, kv_dtype, kv_heads * head_dim).reshape(-1, kv_heads, head_dim)
    kvh = kv_head_of(heads, kv_heads, head_shift)
    s = np.stack([K[:, kvh[h], :] @ q[h] for h in range(heads)]) / np.sqrt(float(head_dim))
    if use_alibi:
        s = s + kq_scale * alibi_slopes(heads, alibi_base_head, alibi_total_heads)[:, None] * np.arange(s.shape[1], dtype=np.float64)[None, :]
    return s


def ref_mix_f64(scores, v_rows, kv_dtype, heads, kv_heads, head_dim, k_index=None, v_index=None, head_shift=0, v64=None):
    """softmax(scores[:, k_index]) . V[v_index] -> float64 [heads * head_dim].  The index arrays (default: every key once, key j with
    value j) are how the mutations are expressed; a key keeps its score (its ALiBi bias included) wherever it goes.  v64: the V rows
    already as float64 [n][kv_dim] (else from the bytes v_rows)."""
    V = (rows_f64(v_rows, kv_dtype, kv_heads * head_dim) if v64 is None else v64).reshape(-1, kv_heads, head_dim)
    if k_index is not None:
        scores = scores[:, k_index]
    e = np.exp(scores - scores.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    if k_index is not None:         # the weight of entry i goes to value row v_index[i] (summed where a row is named twice)
        full = np.zeros((V.shape[0], heads))
        np.add.at(full, k_index if v_index is None else v_index, w.T)
        w = full.T
    kvh = kv_head_of(heads, kv_heads, head_shift)
    return np.concatenate([w[h] @ V[:, kvh[h], :] for h in range(heads)])


def ref_attention_f64(q_rot, k_rows, v_rows, kv_dtype, heads, kv_heads, head_dim, kq_scale=1.0, use_alibi=False,
                      alibi_base_head=0, alibi_total_heads=None):
    """softmax(q . K^T / sqrt(head_dim) [+ alibi]) . V over ALL given rows, float64 [heads * head_dim], no intermediate rounding"""
    s = ref_scores_f64(q_rot, k_rows, kv_dtype, heads, kv_heads, head_dim, kq_scale, use_alibi, alibi_base_head, alibi_total_heads)
    return ref_mix_f64(s, v_rows, kv_dtype, heads, kv_heads, head_dim)


# ----------------------------------------------------------------------------- cases
class Geo:
    """geometry and position-embedding settings of one model"""

    def __init__(self, heads, kv_heads, head_dim, kv_dtype=dt.F16, kq_scale=1.0, use_alibi=0, rope_order=2, partial_rotary=1.0, theta=10000.0):
        self.heads, self.kv_heads, self.head_dim, self.kv_dtype = heads, kv_heads, head_dim, kv_dtype
        self.kq_scale, self.use_alibi, self.rope_order, self.partial_rotary, self.theta = kq_scale, use_alibi, rope_order, partial_rotary, theta
        self.qd, self.kv_dim, self.group = heads * head_dim, kv_heads * head_dim, heads // kv_heads
        self.row_bytes = kv_row_bytes(kv_dtype, self.kv_dim)
        self.attn_kq_scale = 1.0 if use_alibi else kq_scale          # (what both the engine and the reference model hand to the attention)

    def args(self):
        return (self.kv_dtype, self.heads, self.kv_heads, self.head_dim)


def oracle_rope(x16, pos, geo):
    """[heads][head_dim] F16 -> the reference's rotated F16 row (order 0: the model does not call the rotation at all)"""
    x16 = np.ascontiguousarray(x16, np.float16)
    if geo.rope_order == 0:
        return x16.copy()
    return o.rope(x16[None], pos, geo.theta, geo.rope_order, geo.partial_rotary)[0]


def new_token_rows(dqkv16, p, geo):
    """the step's own contribution from its pre-RoPE q | k | v (the engine's "dqkv" buffer): (q_rot F16 [heads][head_dim], K row p bytes,
    V row p bytes) as the reference computes and stores them -- rotation in F16, then the F16 row or its Q8_B32T2 quantisation.  The
    reference reads the step's own key / value back from the cache (oracle/ifa_oracle_model.c: store, then attention over rows 0..p),
    i.e. quantised when the cache is."""
    d = np.ascontiguousarray(dqkv16).view(np.float16).reshape(-1)
    q = d[:geo.qd].reshape(geo.heads, geo.head_dim)
    k = d[geo.qd:geo.qd + geo.kv_dim].reshape(geo.kv_heads, geo.head_dim)
    v = d[geo.qd + geo.kv_dim:geo.qd + 2 * geo.kv_dim]
    q_rot, k_rot = oracle_rope(q, p, geo), oracle_rope(k, p, geo)
    return q_rot, pack_rows(k_rot.reshape(1, -1), geo.kv_dtype)[0], pack_rows(v.reshape(1, -1), geo.kv_dtype)[0]


def probed_keys(p):
    """the cached keys (0 .. p - 1) whose loss a test must notice: the first two, the last, the keys around every entry-bucket
    edge b (b - 1, b, b + 1) and the ends of the 8-key groups those sit in (b - 8, b + 7)"""
    ks = {0, 1, p - 1}
    for b in BUCKETS:
        ks.update((b - 8, b - 1, b, b + 1, b + 7))
    return sorted(j for j in ks if 0 <= j < p)


def _first_heads(q_rot, geo):
    q = np.asarray(q_rot).astype(np.float64).reshape(geo.heads, geo.head_dim)
    return q, q[::geo.group]                                          # all heads, the first query head of every kv group


def flat_keys(q_rot, p, geo):
    """K rows (F16 [p][kv_dim]) whose scores stay within +-FLAT_SCORE for every head: kv head g holds c[j] * q[first head of g], the
    sign of c alternating from key to key (so neighbours never weigh the same) and its size taking two values"""
    q, q0 = _first_heads(q_rot, geo)
    j = np.arange(p)
    target = np.where(j % 2 == 0, 1.0, -1.0) * np.where((j // 2) % 2 == 0, 0.09, 0.07)            # the first head's score of key j
    K = np.zeros((p, geo.kv_heads, geo.head_dim))
    for g in range(geo.kv_heads):
        dots = np.abs(q[g * geo.group:(g + 1) * geo.group] @ q0[g]) / np.sqrt(float(geo.head_dim))     # per unit c: every head of the group
        K[:, g, :] = (target / dots.max())[:, None] * q0[g][None, :]
    return K.reshape(p, geo.kv_dim).astype(np.float16)


def flat_amplitude(n):
    """signature size of the flat family: a lost key moves one output column by ~A / n"""
    return 32.0 if n <= 520 else 64.0


def build_dense(p, geo, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (p, geo.kv_dim)).astype(np.float16), rng.normal(0, 1, (p, geo.kv_dim)).astype(np.float16)


def build_flat(q_rot, p, geo, seed):
    """every key weighs ~1 / n; V row j = N(0, 1) + a signature +-A in column j mod head_dim of every kv head (sign by j / head_dim)"""
    rng = np.random.default_rng(seed)
    V = rng.normal(0, 1, (p, geo.kv_heads, geo.head_dim))
    j = np.arange(p)
    V[j, :, j % geo.head_dim] += (flat_amplitude(p + 1) * np.where((j // geo.head_dim) % 2 == 0, 1.0, -1.0))[:, None]
    return flat_keys(q_rot, p, geo), V.reshape(p, geo.kv_dim).astype(np.float16)


def build_needle_background(q_rot, p, geo, seed):
    rng = np.random.default_rng(seed)
    return flat_keys(q_rot, p, geo), rng.normal(0, 1, (p, geo.kv_dim)).astype(np.float16)


def needle_rows(q_rot, s_bg, bias_bg, j, geo):
    """(K row j bytes, V row j bytes) of the needle at key j over a background whose scores are s_bg ([heads][n], ALiBi bias bias_bg
    included; the step's own key last).  Every kv head's slice is the shortest vector that gives EVERY query head of its group (the
    first one included) the score that makes the key >= NEEDLE_WEIGHT of the head's weight; V is +-4, alternating by column.
    The reference rounds a score to F16 before the softmax, and at a needle's score (~8 .. 12) one F16 step is 2^-7: 0.8 % of a
    weight of 0.05 .. 0.95.  A device whose rotated q differs from the host's in the last bit of one element (another powf / cosf)
    moves the score by up to ~1e-3 -- harmless unless the score sits next to a rounding edge, where the output then jumps by more
    than the reference's own distance from exact math.  So the target scores are put ON the F16 grid and the row is re-solved a few
    times against the scores of the PACKED row.  With F16 rows the scores end within 0.61 of the way from the middle of their rounding
    cell to its edge (the CPU test holds 0.75); a Q8 row moves its scores in steps about as large as the cell (one F16 step of a block
    scale), so there the placement stays arbitrary."""
    q = np.asarray(q_rot).astype(np.float64).reshape(geo.heads, geo.head_dim)
    root = np.sqrt(float(geo.head_dim))
    want = np.zeros(geo.heads)
    for h in range(geo.heads):
        sh = np.delete(s_bg[h], j)
        t = sh.max() + np.log(np.exp(sh - sh.max()).sum()) + np.log(NEEDLE_WEIGHT / (1 - NEEDLE_WEIGHT)) + 0.7 - bias_bg[h, j]
        want[h] = float(np.float16(t)) + float(ulp16(t))                                      # on the F16 grid, not below t
    aim, best = want.copy(), None
    for _ in range(24):         # (every pass rounds a new row: the one whose scores end closest to their targets is kept)
        krow = np.zeros((geo.kv_heads, geo.head_dim))
        for g in range(geo.kv_heads):
            Q = q[g * geo.group:(g + 1) * geo.group]
            krow[g] = Q.T @ np.linalg.solve(Q @ Q.T, aim[g * geo.group:(g + 1) * geo.group] * root)
        packed = pack_rows(krow.reshape(1, -1).astype(np.float16), geo.kv_dtype)
        got = ref_scores_f64(q_rot, packed, *geo.args(), geo.attn_kq_scale)[:, 0]
        miss = float(np.abs(got - want).max())
        if best is None or miss < best[0]:
            best = (miss, packed)
        if miss <= 0.15 * float(ulp16(want).min()):
            break
        aim = aim + (want - got)
    packed = best[1]
    vrow = np.tile(np.where(np.arange(geo.head_dim) % 2 == 0, 4.0, -4.0), geo.kv_heads).astype(np.float16)
    return packed[0], pack_rows(vrow[None], geo.kv_dtype)[0]


_POOL = None        # a few threads for large oracle calls: orc_attention keeps its state in its own mallocs, no globals, and ctypes drops the GIL


def oracle_attention(q_rot, k_rows, v_rows, geo, kv_groups=None):
    """oracle.attention of one query over all given rows -> float64 [heads * head_dim] (kv_groups = (g0, g1): the heads of those kv
    groups only).  Large problems go to the oracle in slices of whole kv groups on a few threads (the heads are independent of each
    other: the same bits as one call)."""
    global _POOL
    n = k_rows.shape[0]
    g = geo

    def run(kv0, kv1):
        per = g.row_bytes // g.kv_heads
        kc = np.ascontiguousarray(k_rows.reshape(n, g.kv_heads, per)[:, kv0:kv1]).reshape(n, -1)
        vc = np.ascontiguousarray(v_rows.reshape(n, g.kv_heads, per)[:, kv0:kv1]).reshape(n, -1)
        if g.kv_dtype == dt.F16:
            kc, vc = kc.view(np.float16), vc.view(np.float16)
        q = np.ascontiguousarray(q_rot[kv0 * g.group:kv1 * g.group])[None]
        return o.attention(q, kc, vc, g.kv_dtype, n, n - 1, (kv1 - kv0) * g.group, kv1 - kv0, g.head_dim, g.attn_kq_scale,
                           bool(g.use_alibi), kv0 * g.group, g.heads)[0].astype(np.float64)

    if kv_groups is not None:
        return run(*kv_groups)
    parts = min(g.kv_heads, 8) if g.heads * n * g.head_dim >= (1 << 19) else 1
    if parts == 1:
        return run(0, g.kv_heads)
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=min(8, max(1, o.usable_cpus())))
    edges = [g.kv_heads * i // parts for i in range(parts + 1)]
    return np.concatenate(list(_POOL.map(lambda i: run(edges[i], edges[i + 1]), range(parts))))


# References already computed, keyed by everything the rows of a case depend on: the bytes of dqkv (sha1), the whole geometry
# (head counts, head size, cache format, ALiBi, rope order / partial rotary / theta, kq_scale), the builders' seed, the position, the
# family and the needle's key.  Entries are immutable (the arrays are read-only) and are never replaced: the routes of one geometry
# meet the same inputs and share them.
_REFS = {}


class Case:
    """one attention problem: q_rot and the n = p + 1 cache rows (bytes), with its references and tolerances"""

    def __init__(self, geo, q_rot, k_rows, v_rows, family, needle=None, scores=None, v64=None, key=None):
        """scores / v64: optional callables that give the float64 scores / V rows cheaper than from the bytes; key: where the
        references of this case are kept for the next route that meets the same inputs (they are never changed)"""
        self.geo, self.q_rot, self.family, self.needle = geo, np.ascontiguousarray(q_rot, np.float16), family, needle
        self.k_rows, self.v_rows = np.ascontiguousarray(k_rows, np.uint8), np.ascontiguousarray(v_rows, np.uint8)
        self.n = self.k_rows.shape[0]
        g = geo
        self._v64 = None
        hit = _REFS.get(key) if key is not None else None
        if hit is None:
            sc = scores() if scores is not None else ref_scores_f64(self.q_rot, self.k_rows, *g.args(), g.attn_kq_scale, bool(g.use_alibi), 0, g.heads)
            self._v64 = v64() if v64 is not None else rows_f64(self.v_rows, g.kv_dtype, g.kv_dim)
            hit = (sc, ref_mix_f64(sc, None, *g.args(), v64=self._v64), self.oracle(self.k_rows, self.v_rows), float(np.abs(self._v64).max()))
            for a in hit[:3]:
                a.setflags(write=False)
            if key is not None:
                _REFS[key] = hit
        self.scores, self.f64, self.orc, self.vmax = hit
        self.d_ref = d_ref(self.orc, self.f64)
        self.tol_orc = 6e-3 * max(1.0, self.vmax)
        self.tol_f64 = max(2.0 * self.d_ref, float(ulp16(np.abs(self.f64).max())))

    @property
    def v64(self):
        if self._v64 is None:
            self._v64 = rows_f64(self.v_rows, self.geo.kv_dtype, self.geo.kv_dim)
        return self._v64

    def oracle(self, k_rows, v_rows, head_roll=0, kv_groups=None):
        g = self.geo
        n = k_rows.shape[0]
        if head_roll:       # the kv head slices of every row moved by head_roll heads: what a wrong head map reads
            per = g.row_bytes // g.kv_heads
            k_rows = np.roll(k_rows.reshape(n, g.kv_heads, per), -head_roll, axis=1).reshape(n, -1)
            v_rows = np.roll(v_rows.reshape(n, g.kv_heads, per), -head_roll, axis=1).reshape(n, -1)
        return oracle_attention(self.q_rot, np.ascontiguousarray(k_rows), np.ascontiguousarray(v_rows), g, kv_groups)

    def weights(self):
        e = np.exp(self.scores - self.scores.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def probes(self):
        if self.family == "needle":
            return [self.needle]
        return probed_keys(self.n - 1)

    # -- mutations: (k_index, v_index) into the n rows
    def mutation(self, kind, j):
        idx = np.arange(self.n)
        if kind == "delete":
            k = np.delete(idx, j)
            return k, k
        if kind == "duplicate":
            k = np.insert(idx, j, j)
            return k, k
        if kind == "swap":          # key j's weight on its neighbour's value and the other way round (the neighbour: the next CACHED key, else the previous, else the step's own)
            nb = j + 1 if j + 1 < self.n - 1 else (j - 1 if j >= 1 else j + 1)
            v = idx.copy()
            v[j], v[nb] = nb, j
            return idx, v
        raise ValueError(kind)

    def mutated_f64(self, kind, j):
        k, v = self.mutation(kind, j)
        return ref_mix_f64(self.scores, None, *self.geo.args(), k_index=k, v_index=v, v64=self.v64)

    def mutated_oracle(self, kind, j):
        """the oracle's output of the case with one fault: key j deleted / duplicated / paired with its neighbour's value, or the kv
        heads of the next group read.  On large problems the fault is in the heads of kv group 0 only and the rest of the output is
        the unmutated oracle's (a fault in one group is the harder one to notice, and one group is a fraction of the oracle's work)."""
        g = self.geo
        part = (0, 1) if g.heads * self.n * g.head_dim >= (1 << 19) else None
        if kind == "wrong_head":
            out = self.oracle(self.k_rows, self.v_rows, head_roll=1, kv_groups=part)
        else:
            k, v = self.mutation(kind, j)
            out = self.oracle(self.k_rows[k], self.v_rows[v], kv_groups=part)
        if part is None:
            return out
        full = self.orc.copy()
        full[:out.size] = out
        return full

    def mutation_kinds(self, j):
        """the mutations that are defined for key j (a single-key context has nothing to lose a key against)"""
        return ("delete", "duplicate", "swap") if self.n >= 2 else ()

    def sensitivity(self):
        """min over the probed keys and mutations of max|mutated float64 - float64| / tol_f64 (inf: nothing to probe)"""
        worst = np.inf
        for j in self.probes():
            for kind in self.mutation_kinds(j):
                worst = min(worst, float(np.abs(self.mutated_f64(kind, j) - self.f64).max()) / self.tol_f64)
        return worst

    def sensitivity_required(self):
        """Exempt from the condition: the dense family past 64 keys (it stands for realistic score spread and the rounding figure),
        and the dense and flat families under ALiBi.  There the reference adds j * slope to the score and rounds the sum to F16 at
        magnitudes up to 64 (ulp 2^-5, i.e. +-1.5 % on a weight), and the steepest head sees the last ~20 keys only: twice that d_ref is
        as large as what a +-0.1 score contrast or a 1 / n weight can move (measured 0.02 x .. 4.3 x the tolerance, test_gqa widths,
        64 .. 257 keys).  Under ALiBi every probed key is covered by its needle case, which meets the condition (>= 7.0 x)."""
        if self.family == "needle":
            return True
        return not (self.n > 64 and self.family == "dense") and not self.geo.use_alibi


def d_ref(orc_out, f64_out):
    """max |oracle.attention - float64|: how far the reference's own rounding points put it from exact math on this input"""
    return float(np.abs(np.asarray(orc_out, np.float64) - np.asarray(f64_out, np.float64)).max())


def make_cases(dqkv16, p, geo, seed=0, families=("dense", "flat", "needle")):
    """every case of position p (n = p + 1 keys) for the step whose pre-RoPE q | k | v is dqkv16.  Yields Case objects; rows 0 .. p - 1 of
    case.k_rows / case.v_rows are what the test writes into the cache, row p what the device must add itself."""
    import hashlib
    q_rot, k_p, v_p = new_token_rows(dqkv16, p, geo)
    base = (hashlib.sha1(np.ascontiguousarray(dqkv16).tobytes()).hexdigest(), geo.kv_dtype, geo.heads, geo.kv_heads, geo.head_dim, geo.use_alibi,
            geo.rope_order, geo.partial_rotary, geo.theta, geo.kq_scale, seed, p)

    def case(K16, V16, family):
        k = np.concatenate([pack_rows(K16, geo.kv_dtype), k_p[None]]) if p else k_p[None]
        v = np.concatenate([pack_rows(V16, geo.kv_dtype), v_p[None]]) if p else v_p[None]
        return Case(geo, q_rot, k, v, family, key=base + (family,))

    empty = np.zeros((0, geo.kv_dim), np.float16)
    if "dense" in families:
        yield case(*(build_dense(p, geo, seed * 7919 + p) if p else (empty, empty)), "dense")
    if p == 0:
        return                                   # one key: the families coincide (the output is the step's own value row)
    if "flat" in families:
        yield case(*build_flat(q_rot, p, geo, seed * 7919 + p + 1), "flat")
    if "needle" in families:
        K, V = build_needle_background(q_rot, p, geo, seed * 7919 + p + 2)
        k_bg = np.concatenate([pack_rows(K, geo.kv_dtype), k_p[None]])
        v_bg = np.concatenate([pack_rows(V, geo.kv_dtype), v_p[None]])
        s_bg = ref_scores_f64(q_rot, k_bg, *geo.args(), geo.attn_kq_scale, bool(geo.use_alibi), 0, geo.heads)
        bias = geo.attn_kq_scale * alibi_slopes(geo.heads)[:, None] * np.arange(p + 1)[None, :] if geo.use_alibi else np.zeros_like(s_bg)
        v64_bg = []
        for j in probed_keys(p):
            kj, vj = needle_rows(q_rot, s_bg, bias, j, geo)
            k2, v2 = k_bg.copy(), v_bg.copy()
            k2[j], v2[j] = kj, vj

            def scores(k2=k2, j=j):
                s2 = s_bg.copy()
                s2[:, j] = ref_scores_f64(q_rot, k2[j:j + 1], *geo.args(), geo.attn_kq_scale)[:, 0] + bias[:, j]
                return s2

            def v64(v2=v2, j=j):
                if not v64_bg:
                    v64_bg.append(rows_f64(v_bg, geo.kv_dtype, geo.kv_dim))
                x = v64_bg[0].copy()
                x[j] = rows_f64(v2[j:j + 1], geo.kv_dtype, geo.kv_dim)[0]
                return x

            c = Case(geo, q_rot, k2, v2, "needle", j, scores=scores, v64=v64, key=base + ("needle", j))
            w = c.weights()[:, j]
            assert w.min() >= NEEDLE_WEIGHT, ("needle weight", p, j, w.min())
            yield c


# ----------------------------------------------------------------------------- the assertions on a device output
def check_att(att, case):
    """att: the attention output under test, [heads * head_dim].  Asserts both bounds; returns max|att - float64| / max(d_ref, ulp / 2),
    the figure the bound 2 is set against."""
    a = np.asarray(att).astype(np.float64).reshape(-1)
    assert np.isfinite(a).all(), "attention output is not finite"
    e_orc = float(np.abs(a - case.orc).max())
    e_f64 = float(np.abs(a - case.f64).max())
    assert e_orc <= case.tol_orc, "att vs oracle.attention: %.3g > %.3g (%s, n %d, needle %s)" % (e_orc, case.tol_orc, case.family, case.n, case.needle)
    assert e_f64 <= case.tol_f64, "att vs float64: %.3g > %.3g (d_ref %.3g; %s, n %d, needle %s)" % (e_f64, case.tol_f64, case.d_ref, case.family, case.n, case.needle)
    return e_f64 / (case.tol_f64 / 2.0)


def check_new_row(k_row_dev, v_row_dev, dqkv16, p, geo):
    """cache row p as the device stored it against the row the reference stores (new_token_rows: oracle.rope of the step's k, the same
    float32 angle recipe as the kernel; then the F16 row or its Q8 blocks).
    F16: every K value within ONE F16 ulp, at the element's own size, of the reference's value; the V row and every column no
    arithmetic touches (a partial rotation's tail, everything without RoPE or at position 0) bit-equal.  One exception, for elements
    smaller than a quarter of the rotated pair's length: one ulp at the PAIR's length (rope_tolerance).  The two sides' powf / cosf
    differ in the last bits of a float32 angle of hundreds of radians, i.e. by up to ~1e-4 rad, and the rotated values by that times
    the pair's length L; two F16 roundings of values that close stay one ulp apart while L x 1e-4 <= ulp(element) ~ 2^-11 |element|,
    i.e. down to |element| ~ L / 5 -- where the two products nearly cancel the element's own ulp shrinks and L x 1e-4 does not.
    Q8: codes within +-1 of the reference's, scales within 0.002 x the largest scale (the bounds of tests/test_gpu_layerwise_oracle.py).
    Returns (values compared, values / codes that differ from the reference's, worst distance in own ulp over the elements held to
    their own ulp, worst distance in pair ulp over the small ones); the last two are 0 for Q8."""
    q_rot, k_ref, v_ref = new_token_rows(dqkv16, p, geo)
    d = np.ascontiguousarray(dqkv16).view(np.float16).reshape(-1)
    k_pre = d[geo.qd:geo.qd + geo.kv_dim].reshape(geo.kv_heads, geo.head_dim)
    if geo.kv_dtype == dt.F16:
        kd = np.ascontiguousarray(k_row_dev).view(np.float16).reshape(geo.kv_heads, geo.head_dim)
        ref = k_ref.view(np.float16).reshape(geo.kv_heads, geo.head_dim).astype(np.float64)
        err = np.abs(kd.astype(np.float64) - ref)
        pair_ulp = rope_tolerance(k_pre, geo.rope_order, geo.partial_rotary)
        small = np.abs(ref) < 256.0 * pair_ulp                  # (an ulp is 2^-10 .. 2^-11 of the length: less than a quarter of the pair's)
        own = np.where(small, 0.0, err / ulp16(ref))
        pair = np.where(small, err / pair_ulp, 0.0)
        assert own.max() <= 1.0, ("F16 K row: more than one ulp from the reference's row", p, float(own.max()))
        assert pair.max() <= 1.0, ("F16 K row: a small element more than one ulp at its pair's length from the reference's row", p, float(pair.max()))
        exact = ref_rope_f64(k_pre, p, geo.theta, geo.rope_order, geo.partial_rotary)
        untouched = exact == k_pre.astype(np.float64)                 # columns the rotation leaves alone (or turns by angle 0: position 0)
        assert np.array_equal(kd[untouched], k_pre[untouched]), ("F16 K row: an unrotated column changed", p)
        assert np.array_equal(np.ascontiguousarray(v_row_dev).view(np.uint8), v_ref), ("F16 V row differs from the step's v", p)
        return int(err.size), int((err != 0).sum()), float(own.max()), float(pair.max())
    diff = 0
    for name, dev, ref in (("K", k_row_dev, k_ref), ("V", v_row_dev, v_ref)):
        a = np.ascontiguousarray(dev, np.uint8).reshape(-1, 34); b = ref.reshape(-1, 34)
        ca, cb = a[:, 2:].view(np.int8).astype(np.int32), b[:, 2:].view(np.int8).astype(np.int32)
        assert np.abs(ca - cb).max() <= 1, ("Q8 %s row codes" % name, p)
        sa = a[:, :2].copy().view(np.float16).astype(np.float32); sb = b[:, :2].copy().view(np.float16).astype(np.float32)
        assert np.abs(sa - sb).max() <= 0.002 * float(sb.max()), ("Q8 %s row scales" % name, p)
        diff += int((ca != cb).sum())
    return 2 * geo.kv_dim, diff, 0.0, 0.0


def check_attq(image, att_dev16, cols):
    """the quantised image of the attention output (xq_image_carve, csrc/ifa_decode_kernels.h: int8 codes [cols], padded to 16 bytes;
    fp32 value of the F16 block scale [cols / 32]; fp32 code sums [cols / 32]) must be the reference quantiser applied to the
    device's OWN att: codes, scales and sums bit for bit"""
    img = np.ascontiguousarray(image, np.uint8)
    nb = cols // 32
    off = (cols + 15) // 16 * 16
    codes = img[:cols].view(np.int8).astype(np.int32)
    scale = img[off:off + 4 * nb].copy().view(np.float32)
    xsum = img[off + 4 * nb:off + 8 * nb].copy().view(np.float32)
    ref = o.quantize_act_q8(np.ascontiguousarray(att_dev16, np.float16).reshape(1, cols)).reshape(nb, 34)
    rc = ref[:, 2:].view(np.int8).astype(np.int32)
    rs = ref[:, :2].copy().view(np.float16).astype(np.float32).reshape(-1)
    assert np.array_equal(codes.reshape(nb, 32), rc), "attq codes"
    assert np.array_equal(scale, rs), "attq scales"
    assert np.array_equal(xsum, rc.sum(axis=1).astype(np.float32)), "attq code sums"


# ----------------------------------------------------------------------------- the matrix both test files walk
N_ONE_WG = (1, 2, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 264, 511, 512, 513, 640)          # one workgroup per head, and the fused launch
N_SPLIT = (1, 2, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 700)             # keys split over workgroups
N_LDS_SPLIT = (1, 9, 257, 700)                                                                        # the split the LDS forces (max_ctx 81920)
N_ODD_HEADS = (65, 257)                                                                             # head_dim 80 / 96
N_VARIANTS = (64, 65, 257)                                                                          # ALiBi / RoPE variants

# name -> (synth shape, overrides, kv dtypes, contexts): the geometries of the GPU matrix (the routes of one geometry share its inputs)
GEOMETRIES = {
    "mha32": ("test_mha", {}, (dt.F16, dt.Q8_B32T2), N_ONE_WG),
    "gqa64": ("test_gqa", {}, (dt.F16, dt.Q8_B32T2), tuple(sorted(set(N_ONE_WG + N_SPLIT)))),
    "tiny48": ("test_tiny", {}, (dt.F16,), N_ONE_WG),
    "wide128": ("llama2_7b", dict(layers=1, ffn=1024, vocab=1000), (dt.F16, dt.Q8_B32T2), tuple(sorted(set(N_ONE_WG + N_SPLIT)))),
    "wide128_kv8": ("llama2_7b", dict(layers=1, ffn=1024, vocab=1000, kv_heads=8), (dt.F16, dt.Q8_B32T2), N_ONE_WG),
    "hd80": ("test_gqa", dict(head_dim=80), (dt.F16,), N_ODD_HEADS),
    "hd96": ("test_gqa", dict(head_dim=96), (dt.F16, dt.Q8_B32T2), N_ODD_HEADS),
    "gqa64_alibi": ("test_gqa", dict(use_alibi=1), (dt.F16, dt.Q8_B32T2), N_VARIANTS),
    "gqa64_rope1": ("test_gqa", dict(rope_order=1), (dt.F16, dt.Q8_B32T2), N_VARIANTS),
    "gqa64_partial": ("test_gqa", dict(partial_rotary=0.5), (dt.F16, dt.Q8_B32T2), N_VARIANTS),
}
_GEO_KEYS = ("use_alibi", "rope_order", "partial_rotary", "kq_scale")


def geometry(name, kv_dtype):
    """(Geo, synth shape name, overrides for synth.build) of one entry of GEOMETRIES"""
    from inferflow_amd.synth import SHAPES
    shape, over, _, _ = GEOMETRIES[name]
    s = dict(SHAPES[shape]); s.update(over)
    geo = Geo(s["heads"], s["kv_heads"], s["head_dim"], kv_dtype, **{k: over[k] for k in _GEO_KEYS if k in over})
    return geo, shape, over


def synthetic_dqkv(geo, seed):
    """a stand-in for the engine's pre-RoPE q | k | v where no device computes one (the CPU test): N(0, 1) values"""
    return np.random.default_rng(seed).normal(0, 1, geo.qd + 2 * geo.kv_dim).astype(np.float16)
