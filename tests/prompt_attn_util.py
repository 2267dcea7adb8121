"""Reference, inputs, faults and assertions of the prompt-attention edge tests (tests/test_prompt_attn_ref_cpu.py on the host,
tests/test_gpu_prompt_attn_edges.py on the device; tests/test_attn_plan_cpu.py uses plan()).

A block of q_tokens queries behind prefix_len cached keys: row t of head h is
    out[t, h] = softmax_j(q[t, h] . K[j, kv(h)] / sqrt(head_dim) [+ kq_scale * j * slope(h)]) . V[j, kv(h)]   over j <= prefix + t, j < n_ctx.
tests/decode_attn_util.py (one query) supplies the packing of cache rows, their float64 reading, the ALiBi slopes, the head map, the F16
ulp and the constants SENSITIVITY, NEEDLE_WEIGHT and FLAT_SCORE; here they are extended to the causal block:

  * Case.f64: that formula in numpy float64, no intermediate rounding.  The mask is a multiplicity array count[t][j] (0 masked, 1 seen,
    2 counted twice) and the K / V pairing an index array vmap[j], so that every fault below is one line (Case.row_f64).
  * families: dense (N(0, 1) everywhere); flat (every key within +-FLAT_SCORE for every query, V row j carries +-A in column j mod
    head_dim, the sign turning with the kv group); needle (per kv group ONE probed key holds >= NEEDLE_WEIGHT of the weight of every
    query that may see it -- the kv groups are independent problems, so a case carries one needle per group).  Every cache row up to
    n_ctx is filled, the rows past a query's causal edge too: a leak moves the row by most of |V needle| or by A / n.
    The needle's score is order-independent: column 0 of every head holds 2.0 in q and 0 in every other key; the needle row is zero
    but for column 0.  q . k is then ONE exact product, and half(alpha * c) the same on every summation order.  A Q8_B32T2 needle row
    has one non-zero code per 32-block and dequantises to scale x 127 on both sides.
  * probed keys, from the plan of the shape (probed_keys), faults (faults_of), and check_rows: the assertions of the device test as a
    function, so that the host test can feed it the oracle's output carrying each fault.

Bounds, per query row over all heads (the project's criterion, docs/decode_attention_edges.md):
    |out - float64| <= max(2 x d_ref, one F16 ulp at max|out|),  d_ref = max|oracle.attention - float64| of that row
    |out - oracle|  <= 6e-3 x max(1, max|V|)"""
import ctypes as C

import numpy as np

import inferflow_amd as ia
import oracle as o
from inferflow_amd import dtypes as dt
from tests import decode_attn_util as D

F16, Q8 = dt.F16, dt.Q8_B32T2
SENSITIVITY, NEEDLE_WEIGHT, FLAT_SCORE = D.SENSITIVITY, D.NEEDLE_WEIGHT, D.FLAT_SCORE
SCALAR, MFMA_LDS, MFMA_WS, TWO_PASS64, TWO_PASS128 = range(5)
KIND_NAMES = ("Scalar", "MfmaLds", "MfmaWorkspace", "TwoPass64", "TwoPass128")
NEVER = 1 << 30
DEFAULT_SETTINGS = (64, NEVER)          # ifa_attention_two_pass_min / _min_keys as the library starts
FORCE_STAGED = (NEVER, NEVER)           # ifa_attention_two_pass_min(0)
FORCE_128 = (64, 0)                     # ifa_attention_two_pass_min_keys(0)
PF_QT, PF_VROW, F2_VROW, LDS_LIMIT = 32, 40, 40, 150 * 1024
Q_NEEDLE = 2.0                          # column 0 of every head of q in the flat and needle families (a power of two)


# ----------------------------------------------------------------------------- the plan
def plan(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, settings=DEFAULT_SETTINGS, rows_mode=0):
    """ifa_attention_plan as a dict"""
    facts = (C.c_int * 10)(kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, settings[0], settings[1], rows_mode)
    out = (C.c_int * 10)()
    ia.check(ia.lib().ifa_attention_plan(facts, 10, out, 10))
    v = list(out)
    return dict(error=v[0], kind=v[1], q_per_wg=v[2], grid=(v[3], v[4]), lds=v[5], sg_nkp=v[6], xcd_remap=v[7],
                ws_bytes=(v[8] & 0xFFFFFFFF) | (v[9] << 32))


def pf_nkp(n_keys):
    return (n_keys + 31) // 32 * 32 + 8


def mfma_lds_bytes(n_ctx, head_dim):
    """the staged kernel's LDS with the score tile in it: [32][pf_nkp] halfs, the transposed V block, 64 bytes"""
    return PF_QT * pf_nkp(n_ctx) * 2 + head_dim * PF_VROW * 2 + 64


def last_lds_ctx(head_dim):
    """the largest n_ctx whose score tile still fits the LDS limit, from the formula: the tile grows by 32 keys at a time"""
    nkp = (LDS_LIMIT - 64 - head_dim * PF_VROW * 2) // (PF_QT * 2)
    return (nkp - 8) // 32 * 32


def f2_col(k):
    """column of key k (0 .. 31) in the two-pass kernels' staged V block: bits 2 and 3 trade places"""
    return (k & 16) | (((k >> 2) & 1) << 3) | (k & 3) | (((k >> 3) & 1) << 2)


# ----------------------------------------------------------------------------- shapes
class Shape:
    """one launch of the device matrix.  kind: the kernel the case is meant for under `settings`; also: further (settings, kind)
    pairs that must take the same input (the references are shared)"""

    def __init__(self, kind, heads, kv_heads, hd, kvd, prefix, qt, n_ctx=None, alibi=0, settings=DEFAULT_SETTINGS, also=(), families=("dense", "flat", "needle"), edge_probes=True, salt=0):
        self.kind, self.heads, self.kv_heads, self.hd, self.kvd, self.prefix, self.qt = kind, heads, kv_heads, hd, kvd, prefix, qt
        self.n_ctx = prefix + qt if n_ctx is None else n_ctx
        self.alibi, self.settings, self.also, self.families, self.edge_probes = alibi, settings, tuple(also), families, edge_probes
        self.kq_scale = 1.0 if alibi else 2.0                    # (as test_attention)
        self.salt = salt                                         # another draw of the same shape (the rows of a batch)

    @property
    def id(self):
        return "%s-h%dkv%d-hd%d-%s-p%d-q%d-n%d%s" % (KIND_NAMES[self.kind], self.heads, self.kv_heads, self.hd, "f16" if self.kvd == F16 else "q8",
                                                     self.prefix, self.qt, self.n_ctx, ("-alibi" if self.alibi else "") + ("-s%d" % self.salt if self.salt else ""))

    def plan(self, settings=None):
        return plan(self.kvd, self.n_ctx, self.qt, self.prefix, self.heads, self.kv_heads, self.hd, settings or self.settings)

    def n_valid(self, t):
        return min(self.n_ctx, self.prefix + t + 1)

    def routes(self):
        return ((self.settings, self.kind),) + self.also

    def tile_nkb(self, qt_tile):
        """32-key blocks of every query tile of qt_tile queries"""
        return [(min(self.n_ctx, self.prefix + min(t0 + qt_tile, self.qt)) + 31) // 32 for t0 in range(0, self.qt, qt_tile)]


def probed_keys(sh):
    """the keys whose loss, doubling or leak a test of this shape must notice, from the plan of its kernel:
    key 0, prefix - 1, prefix and the last key; the diagonal key prefix + t and the key after it for the first and last query of every
    32-query group of the first and the last tile; b - 1, b, b + 1 around every 32-key block edge b that is a stage boundary -- for
    the two-pass kernels every edge (a stage is a pair of blocks, one per parity; an odd count repeats the last), for the staged kernel the
    edges of blocks 1, 4, 5, 8, 9, 12 and 13 (a wave's blocks kb, kb + 4, kb + 8, kb + 12 alternate between two register sets) and of the
    last block of every tile; for the scalar kernel the keys around its 256-thread stride."""
    n, p, qt = sh.n_ctx, sh.prefix, sh.qt
    ks = {0, p - 1, p, n - 1}
    qpw = {SCALAR: 1, MFMA_LDS: 32, MFMA_WS: 32, TWO_PASS64: 64, TWO_PASS128: 128}[sh.kind]
    tiles = sorted({0, (qt - 1) // qpw * qpw})
    for t0 in tiles:
        for g0 in range(t0, min(t0 + qpw, qt), 32):
            for t in (g0, min(g0 + 31, qt - 1)):
                ks.update((p + t, p + t + 1))
    if sh.kind == SCALAR:
        ks.update((255, 256, 257))
    elif sh.edge_probes:
        nkbs = sorted(set(sh.tile_nkb(qpw)))
        if sh.kind in (TWO_PASS64, TWO_PASS128):
            edges = set(range(1, max(nkbs) + 1))
        else:
            edges = {1, 4, 5, 8, 9, 12, 13} | {k - 1 for k in nkbs} | set(nkbs)
        for k in edges:
            ks.update((32 * k - 1, 32 * k, 32 * k + 1))
    return sorted(j for j in ks if 0 <= j < n)


# ----------------------------------------------------------------------------- inputs
def _sig_sign(j, hd, g):
    return np.where((j // hd) % 2 == 0, 1.0, -1.0) * (1.0 if g % 2 == 0 else -1.0)


def _flat_q(sh):
    """q of the flat and needle families: s[t, h] x u with u = +-1 (0 in column 0), column 0 = Q_NEEDLE"""
    hd = sh.hd
    u = np.where(np.arange(hd) % 3 == 0, -1.0, 1.0)
    u[0] = 0.0
    t, h = np.meshgrid(np.arange(sh.qt), np.arange(sh.heads), indexing="ij")
    s = np.array([1.0, -1.0, 0.875, -0.75])[(t + 3 * h) % 4]
    q = s[:, :, None] * u[None, None, :]
    q[:, :, 0] = Q_NEEDLE
    return q.astype(np.float16), u


def _flat_k(sh, u):
    """K rows [n_ctx][kv_dim] (F16): c[j] x u x sqrt(hd) / (hd - 1), so that q . k / sqrt(hd) = s x c[j], |c| = 0.09, 0.07 or 0.03 with the
    sign alternating from key to key and turning with every group of four -- keys 4 .. 7 and 8 .. 11 of a block, which the two-pass
    kernels' column order exchanges, weigh differently, and so do neighbours"""
    j = np.arange(sh.n_ctx)
    c = np.where((j + j // 4) % 2 == 0, 1.0, -1.0) * np.array([0.09, 0.07, 0.09, 0.03])[j % 4]      # (keys 4 k - 1 and 4 k share a sign: 0.03 against 0.09)
    row = c[:, None] * u[None, :] * np.sqrt(float(sh.hd)) / (sh.hd - 1)
    return np.tile(row[:, None, :], (1, sh.kv_heads, 1)).reshape(sh.n_ctx, -1).astype(np.float16)


def flat_amplitude(n):
    """signature size of the flat family: a key's loss moves one output column by ~A / n, its pairing with the neighbour's V row by
    A / n x the contrast of two neighbours' weights (~16 %): decode_attn_util's 32 and 64, and 128 past 2048 keys"""
    return D.flat_amplitude(n) if n <= 2048 else 128.0


def build_inputs(sh, family, seed, needles=None, wants=None):
    """(q F16 [qt][heads][hd], K bytes [n_ctx][row bytes], V bytes) of one case.  needles: {kv group: key}; wants: {kv group: the
    needle's score before the ALiBi bias}"""
    rng = np.random.default_rng(seed)
    n, hd, G = sh.n_ctx, sh.hd, sh.kv_heads
    if family == "dense":
        q = rng.normal(0, 1, (sh.qt, sh.heads, hd)).astype(np.float16)
        K = rng.normal(0, 1, (n, G * hd)).astype(np.float16)
        V = rng.normal(0, 1, (n, G * hd)).astype(np.float16)
        return q, D.pack_rows(K, sh.kvd), D.pack_rows(V, sh.kvd)
    q, u = _flat_q(sh)
    K = _flat_k(sh, u)
    V = rng.normal(0, 1, (n, G, hd))
    if family == "flat":
        j = np.arange(n)
        for g in range(G):
            V[j, g, j % hd] += flat_amplitude(n) * _sig_sign(j, hd, g)
        return q, D.pack_rows(K, sh.kvd), D.pack_rows(V.reshape(n, -1).astype(np.float16), sh.kvd)
    K = K.reshape(n, G, hd).copy()
    for g, j in needles.items():
        K[j, g, :] = 0.0
        K[j, g, 0] = wants[g] * np.sqrt(float(hd)) / Q_NEEDLE
        V[j, g, :] = np.where(np.arange(hd) % 2 == 0, 4.0, -4.0) * (1.0 if g % 2 == 0 else -1.0)
    return q, D.pack_rows(K.reshape(n, -1).astype(np.float16), sh.kvd), D.pack_rows(V.reshape(n, -1).astype(np.float16), sh.kvd)


# ----------------------------------------------------------------------------- float64 reference
def scores_f64(sh, q, k_rows, positions=None, slope_shift=0, head_shift=0):
    """[heads][rows of q][rows of k_rows]: q . K / sqrt(hd) (+ kq_scale * j * slope), every key, masked or not.  positions: the keys' j
    (default 0, 1, ..); slope_shift 1: every head with the slope of the next one; head_shift 1: the kv heads of the next group"""
    K = D.rows_f64(k_rows, sh.kvd, sh.kv_heads * sh.hd).reshape(-1, sh.kv_heads, sh.hd)
    kvh = D.kv_head_of(sh.heads, sh.kv_heads, head_shift)
    q64 = np.asarray(q).astype(np.float64)
    s = np.stack([q64[:, h, :] @ K[:, kvh[h], :].T for h in range(sh.heads)]) / np.sqrt(float(sh.hd))
    if sh.alibi:
        pos = np.arange(s.shape[2], dtype=np.float64) if positions is None else np.asarray(positions, np.float64)
        s = s + sh.kq_scale * D.alibi_slopes(sh.heads, slope_shift, sh.heads)[:, None, None] * pos[None, None, :]
    return s


def causal_count(sh):
    """[qt][n_ctx] multiplicities of the fault-free mask: key j counts once for row t when j <= prefix + t (and j < n_ctx)"""
    return (np.arange(sh.n_ctx)[None, :] < np.array([sh.n_valid(t) for t in range(sh.qt)])[:, None]).astype(np.float64)


def mix_f64(sh, scores, V, count, vmap=None, head_shift=0):
    """scores [heads][rows][n], V float64 [n][kv_heads][hd], count [rows][n] -> [rows][heads * hd]: weights count x exp(score) over the
    counted keys, the weight of key j on V row vmap[j]"""
    s = np.where(count[None] > 0, scores, -np.inf)
    e = np.exp(s - s.max(axis=2, keepdims=True)) * count[None]
    w = e / e.sum(axis=2, keepdims=True)
    Vm = V if vmap is None else V[vmap]
    kvh = D.kv_head_of(sh.heads, sh.kv_heads, head_shift)
    return np.concatenate([w[h] @ Vm[:, kvh[h], :] for h in range(sh.heads)], axis=1)


_POOL = None


def oracle_block(sh, q, k_rows, v_rows, t0=0, t1=None, alibi_base=0):
    """oracle.attention of query rows t0 .. t1 - 1 -> float64 [rows][heads * hd]; large blocks in slices of rows on a few threads (the rows
    are independent of each other: the same bits as one call)"""
    global _POOL
    t1 = sh.qt if t1 is None else t1
    kc, vc = (k_rows.view(np.float16), v_rows.view(np.float16)) if sh.kvd == F16 else (k_rows, v_rows)
    n = k_rows.shape[0]

    def run(a, b):
        return o.attention(np.ascontiguousarray(q[a:b]), kc, vc, sh.kvd, n, sh.prefix + a, sh.heads, sh.kv_heads, sh.hd, sh.kq_scale,
                           bool(sh.alibi), alibi_base, sh.heads).astype(np.float64)

    rows = t1 - t0
    parts = min(8, max(1, o.usable_cpus()), rows) if sh.heads * rows * n * sh.hd >= (1 << 21) else 1
    if parts <= 1:
        return run(t0, t1)
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=8)
    # (later rows see more keys: interleaved edges would balance better, whole slices keep one call per thread)
    edges = [t0 + rows * i // parts for i in range(parts + 1)]
    return np.concatenate(list(_POOL.map(lambda i: run(edges[i], edges[i + 1]), range(parts))))


# ----------------------------------------------------------------------------- cases
_REFS = {}          # (shape id, family, needles) -> Case: the kernels that meet the same input share its references (read-only)


class Case:
    def __init__(self, sh, family, needles=None, background=None):
        self.sh, self.family, self.needles = sh, family, dict(needles or {})
        seed = ((sh.heads * 7 + sh.n_ctx) * 31 + sh.qt) * 17 + sh.salt * 3 + {"dense": 0, "flat": 1, "needle": 2}[family]
        self.count = causal_count(sh)
        self.q, self.k_rows, self.v_rows = build_inputs(sh, family, seed, self.needles, self._needle_scores(background))
        self.V = D.rows_f64(self.v_rows, sh.kvd, sh.kv_heads * sh.hd).reshape(-1, sh.kv_heads, sh.hd)
        self.vmax = float(np.abs(self.V).max())
        t_new = 0
        if background is not None:          # a needle case differs from its background in the needles' columns and rows only
            self.scores = background.scores.copy()
            js = sorted(set(self.needles.values()))
            self.scores[:, :, js] = scores_f64(sh, self.q, self.k_rows[js], positions=js)
            t_new = max(0, min(js) - sh.prefix)
        else:
            self.scores = scores_f64(sh, self.q, self.k_rows)
        self.f64 = mix_f64(sh, self.scores, self.V, self.count)
        if background is not None and t_new > 0:
            self.orc = np.concatenate([background.orc[:t_new], oracle_block(sh, self.q, self.k_rows, self.v_rows, t_new)])
        else:
            self.orc = oracle_block(sh, self.q, self.k_rows, self.v_rows)
        self.d_ref = np.abs(self.orc - self.f64).max(axis=1)                                          # per query row
        self.tol_f64 = np.maximum(2.0 * self.d_ref, D.ulp16(np.abs(self.f64).max(axis=1)))
        self.tol_orc = 6e-3 * max(1.0, self.vmax)
        for a in (self.q, self.k_rows, self.v_rows, self.scores, self.f64, self.orc):
            a.setflags(write=False)
        if family == "flat" or family == "needle":
            vis = self.count[None] > 0
            raw = self.scores - self._bias()
            if family == "needle":
                for g, j in self.needles.items():
                    hs = slice(g * (sh.heads // sh.kv_heads), (g + 1) * (sh.heads // sh.kv_heads))
                    w = self.weights()[hs][:, self.count[:, j] > 0, j]
                    assert w.size == 0 or w.min() >= NEEDLE_WEIGHT, ("needle weight", sh.id, g, j, float(w.min()))
                    raw[hs, :, j] = 0.0
            assert np.abs(np.where(vis, raw, 0.0)).max() <= FLAT_SCORE, ("flat score", sh.id, float(np.abs(np.where(vis, raw, 0.0)).max()))

    def _needle_scores(self, bg):
        """per kv group the least score (before the ALiBi bias) that gives the needle NEEDLE_WEIGHT of the weight of EVERY head of the
        group on EVERY row that sees it, from the background's scores: log-sum-exp of the other visible keys + log(w / (1 - w)), and
        0.05 on top for the F16 rounding of the row.  The row with the most competitors -- the last one -- ends at ~0.9; rows with fewer
        keys beside the needle give it more.  A needle no row sees (past the last query's edge) takes the last row's figure."""
        if not self.needles:
            return {}
        sh, out = self.sh, {}
        group = sh.heads // sh.kv_heads
        bias = bg._bias()
        for g, j in self.needles.items():
            hs = slice(g * group, (g + 1) * group)
            rows = np.nonzero(self.count[:, j] > 0)[0]
            cnt = self.count[rows if rows.size else [sh.qt - 1]].copy()
            cnt[:, j] = 0.0
            s = np.where(cnt[None] > 0, bg.scores[hs][:, rows if rows.size else [sh.qt - 1]], -np.inf)
            m = np.maximum(s.max(axis=2), -1e300)
            lse = np.where(np.isfinite(s.max(axis=2)), m + np.log(np.maximum(np.exp(s - m[:, :, None]).sum(axis=2), 1e-300)), -50.0)
            bj = bias[hs, 0, j][:, None] if sh.alibi else 0.0
            out[g] = float((lse - bj).max() + np.log(NEEDLE_WEIGHT / (1 - NEEDLE_WEIGHT)) + 0.05)
        return out

    def _bias(self):
        sh = self.sh
        if not sh.alibi:
            return 0.0
        return sh.kq_scale * D.alibi_slopes(sh.heads)[:, None, None] * np.arange(sh.n_ctx, dtype=np.float64)[None, None, :]

    def weights(self):
        s = np.where(self.count[None] > 0, self.scores, -np.inf)
        e = np.exp(s - s.max(axis=2, keepdims=True))
        return e / e.sum(axis=2, keepdims=True)

    @property
    def tag(self):
        return "%s %s %s" % (self.sh.id, self.family, sorted(self.needles.items()) if self.needles else "")

    # -- one row with a fault, in float64 and as the oracle computes it
    def row_f64(self, t, count=None, vmap=None, head_shift=0, slope_shift=0):
        sc = self.scores[:, t:t + 1]
        if head_shift or slope_shift:
            sc = scores_f64(self.sh, self.q[t:t + 1], self.k_rows, None, slope_shift, head_shift)
        cnt = self.count[t] if count is None else count
        return mix_f64(self.sh, sc, self.V, cnt[None], vmap, head_shift)[0]

    def row_oracle(self, t, count=None, vmap=None, head_shift=0, slope_shift=0):
        """the oracle on row t with the same fault: the counted keys, each as often as counted, key j with V row vmap[j]"""
        sh = self.sh
        cnt = self.count[t] if count is None else count
        idx = np.repeat(np.arange(sh.n_ctx), cnt.astype(np.int64))
        vidx = idx if vmap is None else np.asarray(vmap)[idx]
        k, v = self.k_rows[idx], self.v_rows[vidx]
        if head_shift:
            per = k.shape[1] // sh.kv_heads
            k = np.roll(k.reshape(len(idx), sh.kv_heads, per), -head_shift, axis=1).reshape(len(idx), -1)
            v = np.roll(v.reshape(len(idx), sh.kv_heads, per), -head_shift, axis=1).reshape(len(idx), -1)
        one = Shape(sh.kind, sh.heads, sh.kv_heads, sh.hd, sh.kvd, len(idx) - 1, 1, len(idx), sh.alibi)
        one.kq_scale = sh.kq_scale
        return oracle_block(one, self.q[t:t + 1], np.ascontiguousarray(k), np.ascontiguousarray(v), alibi_base=slope_shift)[0]


def make_cases(sh, families=None):
    """every case of a shape: dense, flat, and the needle cases -- the probed keys dealt out to the kv groups, one needle per group
    and case (the groups are independent problems), until every probed key has been a needle once"""
    for family in families or sh.families:
        if family != "needle":
            key = (sh.id, family)
            if key not in _REFS:
                _REFS[key] = Case(sh, family)
            yield _REFS[key]
            continue
        if sh.n_ctx < 2:
            continue                                 # one key: nothing to outweigh
        bkey = (sh.id, "needle-background")
        if bkey not in _REFS:
            _REFS[bkey] = Case(sh, "needle", {})
        probes, G = probed_keys(sh), sh.kv_heads
        for i in range(len(probes)):
            if i % G:
                continue
            needles = {g: probes[(i + g) % len(probes)] for g in range(G)}
            key = (sh.id, "needle", tuple(sorted(needles.items())))
            if key not in _REFS:
                _REFS[key] = Case(sh, "needle", needles, background=_REFS[bkey])
            yield _REFS[key]


# ----------------------------------------------------------------------------- faults
def _nb(j, nv):
    return j + 1 if j + 1 < nv else j - 1


def group_edge_rows(sh):
    """the first and the last query of every 32-query group"""
    return sorted({t for g0 in range(0, sh.qt, 32) for t in (g0, min(g0 + 31, sh.qt - 1))})


def fault_blocks(sh):
    """the 32-key blocks the block faults take: the last one, the one before the first query's diagonal, an odd-parity one (block 1 and
    the last odd one)"""
    nkb = (sh.n_valid(sh.qt - 1) + 31) // 32
    blocks = {nkb - 1, (sh.n_valid(0) - 1) // 32 - 1, 1, (nkb - 2) | 1}
    return sorted(b for b in blocks if 0 <= b < nkb)


def faults_of(case):
    """(name, row t, kwargs of Case.row_f64 / row_oracle, the key or first key the fault acts on) of every fault the host test applies
    to a case.  Key faults run on the case's probed keys (a needle case: its needles) at the first and the last row that see the key;
    mask faults at the first and last query of every 32-query group; block faults, the dropped merge and the column order at the first
    and the last query."""
    sh, out = case.sh, []
    n, p, qt = sh.n_ctx, sh.prefix, sh.qt
    keys = sorted(set(case.needles.values())) if case.family == "needle" else probed_keys(sh)
    for j in keys:
        for t in sorted({min(max(0, j - p), qt - 1), qt - 1}):
            nv = sh.n_valid(t)
            if j >= nv or nv < 2:           # (a key past the last query's edge: no row may see it -- the mask faults let it in)
                continue
            for name, mul in (("key deleted", 0.0), ("key counted twice", 2.0)):
                c = case.count[t].copy()
                c[j] = mul
                out.append((name, t, dict(count=c), j))
            vm = np.arange(n)
            vm[j], vm[_nb(j, nv)] = _nb(j, nv), j
            out.append(("key paired with its neighbour's V row", t, dict(vmap=vm), j))
    for t in group_edge_rows(sh):
        nv = sh.n_valid(t)
        if nv < n:
            c = case.count[t].copy()
            c[nv] = 1.0
            out.append(("causal bound + 1", t, dict(count=c), nv))
        if nv >= 2:
            c = case.count[t].copy()
            c[nv - 1] = 0.0
            out.append(("causal bound - 1", t, dict(count=c), nv - 1))
    t_last = qt - 1
    for b in fault_blocks(sh):
        for t in sorted({0, t_last}):
            nv = sh.n_valid(t)
            if 32 * b >= nv or nv <= 32:        # (a row that has this block alone cannot lose it)
                continue
            for name, mul in (("block lost", 0.0), ("block doubled", 2.0)):
                c = case.count[t].copy()
                c[32 * b:min(32 * b + 32, nv)] = mul
                out.append((name, t, dict(count=c), 32 * b))
    if sh.kind in (TWO_PASS64, TWO_PASS128):
        vm = np.minimum(np.array([32 * (j // 32) + f2_col(j % 32) for j in range(n)]), n - 1)
        for t in sorted({0, t_last}):
            if sh.n_valid(t) >= 9:           # (keys 4 .. 7 and 8 .. 11 of a block trade places: a row with fewer keys has nothing to permute)
                out.append(("V block columns unpermuted", t, dict(vmap=vm), None))
            if sh.n_valid(t) > 32:
                out.append(("parities merged without rescaling", t, dict(merge=True), None))
    if qt >= 2:
        for t in sorted({0, qt - 2}):
            out.append(("row of the clamped query", t, dict(clamp=True), None))
    if sh.kv_heads > 1:
        out.append(("kv heads of the neighbouring group", t_last, dict(head_shift=1), None))
    if sh.alibi:
        out.append(("ALiBi slope of the neighbouring head", t_last, dict(slope_shift=1), None))
    return out


def merge_dropped_f64(case, t):
    """row t when the partial sums of the two key-block parities meet WITHOUT rescaling the even blocks' sum to the common maximum:
    each parity has summed exp(s - its own max), and the total takes the even sum as it is.  Equal to the fault-free row wherever the
    even blocks hold the row's maximum."""
    sh = case.sh
    nv = sh.n_valid(t)
    s = case.scores[:, t, :nv]
    odd = (np.arange(nv) // 32) % 2 == 1
    kvh = D.kv_head_of(sh.heads, sh.kv_heads)
    out = []
    for h in range(sh.heads):
        se, so, M = s[h][~odd], s[h][odd], s[h].max()
        tot = np.exp(se - se.max()).sum() + np.exp(so - M).sum()
        out.append((np.exp(s[h] - M) / tot) @ case.V[:nv, kvh[h], :])
    return np.concatenate(out)


def faulty_row(case, t, kw, oracle):
    """row t with the fault kw, in float64 or as the oracle computes it.  The clamp hands over row q_tokens - 1 of the same output; the
    dropped merge has no expression in the oracle's inputs, so its oracle row is the oracle's own plus the float64 displacement."""
    if kw.get("clamp"):
        return (case.orc if oracle else case.f64)[case.sh.qt - 1]
    if kw.get("merge"):
        d = merge_dropped_f64(case, t)
        return case.orc[t] + (d - case.f64[t]) if oracle else d
    return (case.row_oracle if oracle else case.row_f64)(t, **kw)


def sensitivity_required(case, name, t, j):
    """Where |faulty float64 row - float64 row| >= SENSITIVITY x the row's bound is asserted (and the oracle's output carrying the fault
    must be rejected).  As in docs/decode_attention_edges.md, exempt are the dense family past 64 keys (it stands for realistic score
    spread and the rounding figure) and the dense and flat families under ALiBi (the reference rounds score + bias to F16 where one step
    is percents of a weight, so 2 x d_ref is as large as what a +-0.1 contrast or a 1 / n weight moves); every probed key is covered by
    its needle case.  Two faults do not depend on a single key's weight and are asserted on the dense family at every size: the clamped
    row (another query's whole result) and, under ALiBi, the neighbouring head's slope (it decides which keys a head sees at all).
    A needle case has ONE heavy key per kv group (sensitivity_required's comments give the arithmetic of what it cannot show), so it answers for the faults that touch that key: the key faults, a causal bound that
    moves across it, a block that holds it, the dropped merge when it lies in an odd block (the even sum is then the one that needs the
    rescaling), and the neighbouring group's kv heads (another needle, or none).  The faults that touch no single key -- blocks without
    the needle, the column order, the clamp -- are asserted on the flat family of the same shape."""
    f, sh = case.family, case.sh
    if name == "ALiBi slope of the neighbouring head":
        return f == "dense" and sh.n_valid(t) > 8
    if name == "row of the clamped query" and f == "dense":
        return True
    if f == "needle":
        nd = set(case.needles.values())
        if name in ("key counted twice", "block doubled") and (t != sh.qt - 1 or sh.alibi):
            # counting a weight w twice makes it 2 w / (1 + w): on the first row that sees a needle, with few keys beside it, twice nearly
            # all the weight is nearly all of it, so this is asserted on the last row (w ~ 0.9: a step of 0.047 x |V needle - rest|).
            # Under ALiBi not at all: the reference rounds score + bias to F16 at 32 .. 200 (steps of 2^-5 .. 2^-3), the needle's weight
            # carries w (1 - w) x that, and 2 x d_ref is then as large as the step.  The counting of keys does not depend on the bias:
            # the shapes without ALiBi on the same kernel answer for it.
            return False
        if name in ("key deleted", "key counted twice", "key paired with its neighbour's V row", "causal bound + 1", "causal bound - 1"):
            return j in nd
        if name in ("block lost", "block doubled"):
            return any(32 * (j // 32) <= k < 32 * (j // 32) + 32 and k < sh.n_valid(t) for k in nd)
        if name == "parities merged without rescaling":
            return any((k // 32) % 2 == 1 and k < sh.n_valid(t) for k in nd)
        if name == "kv heads of the neighbouring group":
            return len(nd) > 1 and any(k < sh.n_valid(t) for k in nd)
        return False
    if sh.alibi:
        return False
    if name == "parities merged without rescaling":
        return False                    # (the flat scores' maximum is in both parities; dense: wherever it falls)
    if f == "dense":
        return sh.n_ctx <= 64
    return True


# ----------------------------------------------------------------------------- the assertions on a device output
def check_rows(out, case):
    """out: [qt][heads * hd] under test.  Asserts both bounds on every query row; returns per row max|out - float64| / max(d_ref, ulp / 2),
    the figure the bound 2 is set against."""
    a = np.asarray(out).astype(np.float64).reshape(case.sh.qt, -1)
    assert np.isfinite(a).all(), "attention output is not finite (%s)" % case.tag
    e_orc = np.abs(a - case.orc).max(axis=1)
    e_f64 = np.abs(a - case.f64).max(axis=1)
    t = int(np.argmax(e_orc))
    assert e_orc[t] <= case.tol_orc, "out vs oracle.attention: %.3g > %.3g at row %d (%s)" % (e_orc[t], case.tol_orc, t, case.tag)
    r = e_f64 / case.tol_f64
    t = int(np.argmax(r))
    assert r[t] <= 1.0, "out vs float64: %.3g > %.3g at row %d (d_ref %.3g; %s)" % (e_f64[t], case.tol_f64[t], t, case.d_ref[t], case.tag)
    return e_f64 / (case.tol_f64 / 2.0)


# ----------------------------------------------------------------------------- the device matrix
def _sh(*a, **k):
    return Shape(*a, **k)


STAGED_TOO = ((FORCE_STAGED, MFMA_LDS),)
ALL_THREE = ((FORCE_STAGED, MFMA_LDS), (FORCE_128, TWO_PASS128))

# TwoPass64: queries 64 .. 161 (last tiles of 64, 1, 31, 32, 33, 63 queries), prefixes 0 .. 200; the first tile has 2 blocks behind prefix 0
# and 3 behind 1 .. 64; the last tile's block count is odd and even (test_prompt_attn_ref_cpu.py checks the coverage); from 128 queries on
# the same inputs go to the 128-query variant and to the staged kernel, below that to the staged kernel
TWO_PASS = [
    _sh(TWO_PASS64, 8, 2, 64, F16, 0, 64, also=STAGED_TOO),
    _sh(TWO_PASS64, 8, 8, 64, Q8, 1, 65, also=STAGED_TOO),
    _sh(TWO_PASS64, 4, 1, 128, F16, 31, 95),
    _sh(TWO_PASS64, 6, 3, 64, Q8, 32, 96, alibi=1),
    _sh(TWO_PASS64, 8, 4, 128, Q8, 33, 97),
    _sh(TWO_PASS64, 6, 6, 64, F16, 63, 127),
    _sh(TWO_PASS64, 8, 4, 64, F16, 64, 128, also=ALL_THREE),
    _sh(TWO_PASS64, 4, 2, 128, Q8, 200, 129, also=ALL_THREE),
    _sh(TWO_PASS64, 8, 8, 64, F16, 0, 161, alibi=1, also=ALL_THREE),
    _sh(TWO_PASS64, 4, 4, 128, F16, 1, 161, also=ALL_THREE),
    _sh(TWO_PASS64, 8, 2, 64, F16, 33, 65, n_ctx=33 + 65 + 40),             # more cache rows than the last query may see
]
# MfmaLds: 4 .. 63 queries, 1 / 4 / 5 / 8 / 9 / 12 / 13 key blocks in a tile, n_valid of the last query = 0, 1 and 7 mod 8
MFMA = [
    _sh(MFMA_LDS, 8, 8, 32, F16, 0, 4),
    _sh(MFMA_LDS, 6, 2, 64, Q8, 123, 5),             # 128 keys: 4 blocks, n_valid % 8 == 0
    _sh(MFMA_LDS, 4, 1, 128, F16, 98, 31),           # 129 keys: 5 blocks, % 8 == 1
    _sh(MFMA_LDS, 8, 2, 32, Q8, 224, 32),            # 256 keys: 8 blocks
    _sh(MFMA_LDS, 8, 4, 64, F16, 224, 33, alibi=1),  # 257 keys: 9 blocks in the second tile, 8 in the first
    _sh(MFMA_LDS, 4, 2, 128, Q8, 320, 63),           # 383 keys: 12 blocks (% 8 == 7), the first tile 11
    _sh(MFMA_LDS, 8, 8, 64, F16, 322, 63),           # 385 keys: 13 blocks, the first tile 12
    _sh(MFMA_LDS, 6, 3, 32, F16, 31, 33),            # an unaligned short prefix: 2 blocks, then 3 for ONE query
]


def workspace_shapes():
    """per head_dim: the plan's last n_ctx on the LDS tile and the next one, 4 and 40 queries behind the prefix (2 heads, 1 kv head)"""
    out = []
    for hd, kvd in ((32, F16), (64, Q8), (128, F16)):
        last = last_lds_ctx(hd)
        for n, kind in ((last, MFMA_LDS), (last + 1, MFMA_WS)):
            for qt in (4, 40):
                # (the block edges of the prefix are those of the 4-query shape on the same n_ctx: probed there, every case is 10 x cheaper)
                out.append(_sh(kind, 2, 1, hd, kvd, n - qt, qt, edge_probes=qt == 4))
    return out


# Scalar: 1 .. 3 queries around the 256-thread stride, and head sizes no MFMA kernel takes
SCALAR_SHAPES = ([_sh(SCALAR, 8 if n % 2 else 6, 2, 64 if q != 2 else 32, F16 if (n + q) % 2 else Q8, n - q, q) for q in (1, 2, 3) for n in (1, 2, 255, 256, 257, 513) if n >= q]
                 + [_sh(SCALAR, 4, 2, 48, F16, 13, 5), _sh(SCALAR, 4, 4, 80, F16, 250, 5), _sh(SCALAR, 4, 2, 48, F16, 0, 70), _sh(SCALAR, 4, 2, 80, F16, 190, 70, alibi=1)])


def device_matrix():
    return TWO_PASS + MFMA + workspace_shapes() + SCALAR_SHAPES


ROWS_CTX = (1, 2, 255, 256, 257, 600)
# ifa_attention_rows: (contexts of the rows in order, heads, kv_heads, hd, kv dtype, alibi): the shortest row first and last
ROWS_BATCHES = [
    ((1,), 8, 2, 64, F16, 0), ((600,), 4, 4, 128, Q8, 0),
    ((1, 600), 8, 8, 64, Q8, 0), ((257, 1), 6, 2, 32, F16, 0),
    ((1, 256, 600, 255, 2), 8, 4, 64, F16, 0), ((2, 257, 255, 600, 1), 4, 2, 128, Q8, 1),
    ((1, 2, 255, 256, 257, 600, 256, 1), 8, 2, 64, F16, 0), ((2, 600, 1, 257, 256, 255, 600, 1), 4, 2, 80, F16, 0),
]


def row_shape(n, heads, kv_heads, hd, kvd, alibi, r=0):
    """row r of a rows batch as a one-query case over its own n keys (r: its own draw of the inputs)"""
    return Shape(SCALAR, heads, kv_heads, hd, kvd, n - 1, 1, n, alibi, salt=r)


def rows_batch_shapes(batch):
    ctxs, heads, kv_heads, hd, kvd, alibi = batch
    return [row_shape(n, heads, kv_heads, hd, kvd, alibi, r) for r, n in enumerate(ctxs)]
