"""The device-routed mixture-of-experts layer on routings the test DESIGNS (docs/moe_layer_edges.md): the models, the routings and their margins,
the reference of every launch of the layer from the inputs the device had, the assertion, and the faults that assertion must reject.
tests/test_moe_layer_ref_cpu.py runs the host half, tests/test_gpu_moe_layer_edges.py the device half.

How a routing is designed.  Wv and Wo are zero, so the FFN input of row i is embedding row i.  The first E columns of an embedding row are a
code, the others N(0, 1).  Gate row e is G_GATE x the unit vector e and the FFN norm weight is 1 on the code columns, so the logit of expert e
is G_GATE x (the normalised code e) exactly: one non-zero term in the gate product, a power of two as factor.  Codes: CODE_HI / CODE_LO for the
two experts a row selects (weights ~0.8 / ~0.2), CODE_OFF for the others, CODE_ONLY for the one expert of a row whose other slot is dropped
(every other probability rounds to 0), equal codes for ties.

Bound of a product launch (the exact-input criterion of docs/decode_gemv_edges.md): every element within max(2 x d_ref, one F16 ulp at |out|)
of float64, d_ref = max|oracle - float64| over the LAUNCH: all groups of one list (tiles, smalls, singles) of one product."""
from dataclasses import dataclass, field

import numpy as np

import oracle as o
from inferflow_amd import dtypes as dt, worker as W
from tests import moe_lists_util as M
from tests import rows_gemm_util as U
from tests.decode_attn_util import ulp16
from tests.decode_gemv_util import SENSITIVITY, act_f64, q8_parts

DIM, G_GATE = 256, 2.0
CODE_HI, CODE_LO, CODE_OFF, CODE_ONLY = 6.0, 5.0, -6.0, 64.0
W_STD = U.W_STD
WD = dt.Q4_B32T1A
PLAN_KEYS = ("kind", "router", "tile_rows", "small_max", "max_tiles", "smalls_mo", "side_stream")
T_OF = {0: W.T_W1, 1: W.T_W3, 2: W.T_W2}              # which: the order of the tiled pointer table {w1, w3, w2}


# ----------------------------------------------------------------------------- rows of a routing
def pair(a, b):
    """expert a with the larger weight, b with the smaller"""
    return {a: CODE_HI, b: CODE_LO}


def only(a):
    """expert a alone: the second pick's probability is 0, its slot is dropped"""
    return {a: CODE_ONLY}


def tie(*ids, above=None):
    """equal codes on ids (the lowest ids win what is left of the top k); above: one expert clearly in front of them"""
    r = {e: CODE_HI for e in ids}
    if above is not None:
        r[above] = CODE_HI + 1.0
    return r


def is_tie(codes):
    v = sorted(codes.values())
    return any(a == b for a, b in zip(v, v[1:]))


def expected_sel(codes, E, K):
    """the routers' row: the top K by (code descending, id ascending), only the CODE_ONLY experts where there is one, ascending ids, -1 behind"""
    full = [(-codes.get(e, CODE_OFF), e) for e in range(E)]
    top = sorted(full)[:K]
    if any(c == -CODE_ONLY for c, _ in top):
        top = [t for t in top if t[0] == -CODE_ONLY]
    ids = sorted(e for _, e in top)
    return ids + [-1] * (K - len(ids))


@dataclass
class Routing:
    """one step: mode batch (decode_batch of n rows, caller_norm 1) or prompt (forward of n tokens); rows: {expert: code} per row"""
    name: str
    mode: str
    E: int
    K: int
    rows: list
    ffn: int = 512
    seed: int = 0
    dim: int = DIM

    @property
    def n(self):
        return len(self.rows)

    @property
    def V(self):
        return max(32, self.n)

    @property
    def id(self):
        return "%s-E%d-n%d-f%d-%s%s%s" % (self.mode, self.E, self.n, self.ffn, self.name, "" if self.K == 2 else "-k%d" % self.K, "" if self.dim == DIM else "-d%d" % self.dim)

    def sel(self):
        return np.array([expected_sel(r, self.E, self.K) for r in self.rows], np.int32)

    def counts(self):
        s = self.sel()
        return np.bincount(s[s >= 0], minlength=self.E)


def from_counts(name, mode, E, K, n, counts, ffn=512, seed=0):
    """rows in which expert e is selected counts[e] times; a row with two experts is a pair (the larger weight alternating), with one an `only`"""
    rng = np.random.default_rng(17 + n + 3 * E + seed)
    sel = M._place(list(counts) + [0] * (E - len(counts)), n, K, rng)
    rows = []
    for t in range(n):
        ids = [int(e) for e in sel[t] if e >= 0]
        assert 1 <= len(ids) <= 2, "every row needs an expert"
        rows.append(only(ids[0]) if len(ids) == 1 else pair(*(ids if t % 2 == 0 else ids[::-1])))
    return Routing(name, mode, E, K, rows, ffn, seed)


def prompt_rows(E, T):
    """every row on expert 0 as first choice; the second choice: expert E - 2 for rows 0 and 1 (a 2-row expert), expert E - 1 for the last row
    (alone there), the experts 1 .. E - 3 in turn for the rest"""
    rows = []
    mid = list(range(1, E - 2)) or [1]
    for t in range(T):
        second = E - 1 if t == T - 1 else (E - 2 if t < 2 and T >= 4 else mid[t % len(mid)])
        rows.append(pair(0, second))
    return rows


def ffn_norm_weight(E, dim=DIM):
    w = U.norm_weight(dim).copy()
    w[:E] = 1.0
    return w


def embedding(rc):
    """[V][dim] F16: row i = code of routing row i (rows past n: a pair on experts 0, 1), N(0, 1) elsewhere"""
    rng = np.random.default_rng(9000 + rc.n + 31 * rc.E + rc.seed + len(rc.name))
    Em = rng.normal(0, 1, (rc.V, rc.dim)).astype(np.float16)
    Em[:, :rc.E] = CODE_OFF
    for i in range(rc.V):
        for e, c in (rc.rows[i] if i < rc.n else pair(0, 1)).items():
            Em[i, e] = c
    return Em


def gate_weight(E, dim=DIM):
    g = np.zeros((E, dim), np.float16)
    g[np.arange(E), np.arange(E)] = G_GATE
    return g


def host_router(rc):
    """the router of the step in the oracle's F16 steps: hn, logits, probabilities [n][E] F16, sel [n][K], weights (F16 bits of oracle.moe_topk)"""
    Em = embedding(rc)[:rc.n]
    hn = o.rmsnorm(Em, ffn_norm_weight(rc.E, rc.dim), None, 0.0, 1e-5)
    logits = (hn[:, :rc.E].astype(np.float32) * np.float32(G_GATE)).astype(np.float16)
    probs = o.softmax(logits.reshape(1, rc.n, rc.E).copy()).reshape(rc.n, rc.E)
    sel, w = route_of_probs(probs, rc.K)
    return dict(hn=hn, logits=logits, probs=probs, sel=sel, w=w)


def route_of_probs(probs16, K, norm=True):
    """oracle.moe_topk of every row in the routers' form: ascending ids, -1 / weight 0 behind"""
    T = probs16.shape[0]
    sel, w = np.full((T, K), -1, np.int32), np.zeros((T, K), np.float16)
    for t in range(T):
        idx, wt = o.moe_topk(probs16[t].astype(np.float32), K, norm)
        order = np.argsort(idx, kind="stable")
        sel[t, :len(idx)] = idx[order]; w[t, :len(idx)] = wt[order].astype(np.float16)
    return sel, w


def check_margins(rc):
    """the design margins the device test relies on; returns (smallest logit gap, smallest kept probability, largest dropped probability,
    smallest weight difference) over the rows that test no tie"""
    r = host_router(rc)
    dim = rc.dim
    assert np.array_equal(r["sel"], rc.sel()), (rc.id, "the oracle's routing of the designed rows is not the designed routing")
    lg = r["logits"].astype(np.float64)
    assert np.abs(lg).max() <= G_GATE * np.sqrt(dim)
    ex = np.exp(lg - lg.max(axis=1, keepdims=True)); p64 = ex / ex.sum(axis=1, keepdims=True)
    gap, kept, dropped, wdiff = np.inf, np.inf, 0.0, np.inf
    for t, codes in enumerate(rc.rows):
        want = [e for e in rc.sel()[t] if e >= 0]
        rest = [e for e in range(rc.E) if e not in want]
        kept = min(kept, p64[t, want].min())
        if len(want) < rc.K:                                 # the dropped slot: the best of the rest
            dropped = max(dropped, p64[t, rest].max())
        if is_tie(codes):
            continue
        if rest:
            gap = min(gap, lg[t, want].min() - lg[t, rest].max())
        w = np.sort(r["w"][t, :len(want)].astype(np.float64))
        if len(w) > 1:
            wdiff = min(wdiff, np.diff(w).min())
    assert gap >= 0.5, (rc.id, "selected and unselected logits", gap)
    assert kept >= 1e-4 and dropped <= 1e-6, (rc.id, kept, dropped)
    assert wdiff >= 0.05, (rc.id, "kept weights", wdiff)
    return gap, kept, dropped, wdiff


# ----------------------------------------------------------------------------- the cases
def batch_singles_cases():
    """batched n = 2, 4, 8 on 8 experts, top 2 (no tile possible: the singles route)"""
    c = []
    for n in (2, 4, 8):
        spread = [1] * min(8, 2 * n) if n < 8 else [1] * 8
        groups = {2: [1, 2, 0, 1], 4: [1, 3, 4], 8: [1, 5, 1, 3, 2, 4]}[n]
        drop = {2: [1, 1, 1], 4: [2, 1, 2, 1], 8: [4, 3, 1, 2, 1, 1]}[n]
        c.append(from_counts("spread", "batch", 8, 2, n, spread))
        c.append(from_counts("two", "batch", 8, 2, n, [n, n]))
        c.append(from_counts("groups", "batch", 8, 2, n, groups))
        c.append(from_counts("drop", "batch", 8, 2, n, drop))
        c.append(from_counts("ends", "batch", 8, 2, n, [n, 0, 0, 0, 0, 0, 0, n]))
    c.append(from_counts("groups", "batch", 8, 2, 4, [1, 3, 4], ffn=4352))       # W2 of the 4-row group: whole-row staging; 3 rows: the same
    c.append(from_counts("groups", "batch", 8, 2, 8, [1, 5, 1, 3, 2, 4], ffn=4352))      # 5 rows: the chunk loop
    return c


def batch_grouped_cases():
    """batched n = 9, 16, 32 (a tile is possible: the grouped route)"""
    return [from_counts("tile9-small8-single", "batch", 8, 2, 9, [9, 8, 1]),
            from_counts("tile9-smalls-single", "batch", 8, 2, 16, [9, 8, 1, 2, 3, 4, 5]),
            from_counts("two", "batch", 8, 2, 32, [32, 32]),
            from_counts("even", "batch", 8, 2, 32, [8] * 8)]


def prompt_cases():
    return [Routing("first0", "prompt", 8, 2, prompt_rows(8, T)) for T in (2, 8, 9, 17, 33, 65, 129)] + [Routing("first0", "prompt", 4, 2, prompt_rows(4, 193))]


def tie_cases():
    """8 rows each: two equal at the top, three equal for two places (the lowest two ids), two equal behind a clear first, and next to each a
    row with a dropped slot (its second pick is a tie among seven probabilities of 0)"""
    rows = [tie(2, 5), tie(6, 1, 3), tie(7, 4, above=0), only(3), tie(0, 7), tie(5, 6, 7), tie(1, 2, above=6), only(0)]
    return [Routing("ties", "batch", 8, 2, rows), Routing("ties", "prompt", 8, 2, rows)]


def router_cases():
    """8 batched rows on other expert counts and top k: 5 and 9 experts (waves clamped to E - 1; an expert past the first round of 8 waves), 64
    experts, top 1, top 8 (8 distinct weights cannot differ by 0.05 each: its rows are ties -- 8 equal, 9 equal for 8 places -- and dropped
    slots), and dim 4096 / 4128 (512 / 516 16-byte chunks of a row: the RMS sum's second pass, the gate product's second round and its clamp)"""
    def rows(E):
        last = E - 1
        return [pair(0, last), pair(last, 1), only(last), pair(E // 2, last), tie(0, last), tie(1, 2, last), only(0), pair(last - 1, last)]
    c = [Routing("router", "batch", E, 2, rows(E)) for E in (5, 9, 64)]
    c.append(Routing("router", "batch", 8, 1, rows(8)))
    ids = [3, 9, 17, 25, 33, 41, 49, 57, 63]
    c.append(Routing("router", "batch", 64, 8, [tie(*ids[:8]), tie(*ids), only(63), tie(*range(8)), tie(*range(56, 64)), only(0), tie(*ids[1:]), tie(*range(20, 29))]))
    c += [Routing("router", "batch", 8, 2, rows(8), dim=d) for d in (4096, 4128)]
    return c


def all_cases():
    return batch_singles_cases() + batch_grouped_cases() + prompt_cases() + tie_cases() + router_cases()


OPTION_SETS = (("default", {}), ("moe_singles0", {"moe_singles": 0}), ("rows_mo0", {"rows_mo": 0}), ("moe_overlap0", {"moe_overlap": 0}),
               ("router_ops", {"moe_router_fused": 0}))


def plan_facts(rc, opts=None, have_mo=1):
    """the facts of the model of a case (every expert Q4_B32T1A, tiled, reference-layout and -- once a batched step has run -- MO tables)"""
    opts = opts or {}
    batch = rc.mode == "batch"
    f = dict(T=rc.n, experts=rc.E, top_k=rc.K, dim=rc.dim, ffn=rc.ffn, w_dtype=WD, w_ax8=1, w_q4=1, full_quant_gemv=1, norm_kind=0, gate_f16=1, gate_cols_match=1,
             has_ffn_norm=1, experts_uniform=1, have_table=1, have_table_aos=1, have_table_mo=int(have_mo and opts.get("rows_mo", 1)), moe_device=1,
             moe_router_fused=1, moe_singles=1, moe_overlap=1, gemm_rows=1, rows_mo=1, rows_use_mfma=1, rows_mfma_ok=1, rows_q4_ok=1, singles_ok=1, caller_norm=int(batch))
    f.update(opts)
    return f


def expected_plan(rc, opts=None, have_mo=1):
    """the plan the case is designed for, written down (not computed by the code under test)"""
    opts = opts or {}
    n, cap, batch = rc.n, rc.n * rc.K, rc.mode == "batch"
    mo = int(have_mo and opts.get("rows_mo", 1))
    small_max = 8 if cap <= 8 * rc.E else 0
    max_tiles = 0 if (small_max and n <= small_max) else cap // (128 if cap // rc.E >= 96 else 64) + rc.E
    singles = bool(opts.get("moe_singles", 1)) and max_tiles == 0 and mo
    return dict(kind="device_singles" if singles else "device_grouped", router="fused" if batch and n <= 32 and opts.get("moe_router_fused", 1) else "ops",
                tile_rows=128 if cap // rc.E >= 96 else 64, small_max=small_max, max_tiles=max_tiles, smalls_mo=int(bool(mo and small_max)),
                side_stream=int(singles and bool(opts.get("moe_overlap", 1))))


# ----------------------------------------------------------------------------- weights
class Expert:
    """W1, W3, W2 of one expert in the reference byte layout with both float64 views: `half` -- the half-rounded dequantised value the F16
    activation kernels multiply -- and `f32` -- scale x code + base as the int8 path decodes it"""

    def __init__(self, tensors):
        self.t = {}
        for which, (d, data, rows, cols) in tensors.items():
            self.t[which] = (d, np.ascontiguousarray(data, np.uint8).reshape(rows, dt.row_bytes(d, cols)), rows, cols)
        self._w = {}

    def w64(self, which, view):
        if (which, view) not in self._w:
            d, data, rows, cols = self.t[which]
            self._w[(which, view)] = o.dequantize(d, data, cols, out_f32=(view == "f32")).astype(np.float64)
        return self._w[(which, view)]


def host_experts(E, ffn, dim=DIM, seed=0):
    """experts of the host test: N(0, W_STD) quantised by the oracle"""
    out = []
    for e in range(E):
        t = {}
        for which, (rows, cols) in ((0, (ffn, dim)), (1, (ffn, dim)), (2, (dim, ffn))):
            rng = np.random.default_rng(100000 + 16 * e + which + seed)
            t[which] = (WD, o.quantize(WD, rng.normal(0, W_STD, (rows, cols)).astype(np.float16)), rows, cols)
        out.append(Expert(t))
    return out


# ----------------------------------------------------------------------------- the reference of a step's launches
@dataclass
class Group:
    kind: str                        # tile | small | single
    expert: int
    row0: int
    nrows: int


@dataclass
class LaunchRef:
    """one product of one list: the rows it writes, float64 and the oracle's value of each, the bound"""
    name: str                        # e.g. tiles.g1
    rows: np.ndarray
    f64: np.ndarray
    orc: np.ndarray
    d_ref: float = 0.0
    bound: np.ndarray = field(default=None)


def groups_of(L):
    g = [Group("tile", *[int(v) for v in r[:3]]) for r in L.tiles] + [Group("small", *[int(v) for v in r[:3]]) for r in L.smalls]
    g += [Group("single", int(r[0]), int(r[1]), 1) for r in L.singles]
    return sorted(g, key=lambda x: x.row0)


class LayerRef:
    """experts: [Expert]; L: the lists (M.Lists); gin [entries][dim] F16: the gathered rows the device had; g1 [entries][ffn] F16: the gated
    rows the device had (input of W2).  act_kind 0."""

    def __init__(self, experts, L, gin, g1, act_kind=0):
        self.ex, self.L, self.act = experts, L, act_kind
        n = int(L.counts[0])
        self.gin, self.g1 = np.ascontiguousarray(gin[:n], np.float16), np.ascontiguousarray(g1[:n], np.float16)
        self.groups = groups_of(L)
        assert sum(g.nrows for g in self.groups) == n

    # -- one group's product in float64 / by the oracle, in the arithmetic of its list
    def x64(self, kind, X16):
        if kind != "single":
            return X16.astype(np.float64)
        q = o.quantize_act_q8(np.ascontiguousarray(X16, np.float16))
        out = np.empty(X16.shape)
        for r in range(X16.shape[0]):
            codes, xs = q8_parts(q[r], X16.shape[1])
            out[r] = (codes * xs[:, None]).reshape(-1)
        return out

    def pre64(self, kind, e, which, X16):
        return self.x64(kind, X16) @ self.ex[e].w64(which, "f32" if kind == "single" else "half").T

    def orc16(self, kind, e, which, X16):
        d, data, rows, cols = self.ex[e].t[which]
        X16 = np.ascontiguousarray(X16, np.float16)
        if kind != "single":
            return o.gemm_f16x(d, data, rows, cols, X16, None)
        q = o.quantize_act_q8(X16)
        return np.stack([o.gemv_ax8(d, data, rows, cols, q[r]) for r in range(X16.shape[0])])

    def glu64(self, p1, p3):
        return act_f64(p1, self.act) * p3

    def launches(self, with_g3=True):
        """{name: LaunchRef} of the step: per list the gated product (g1), W3's product (g3: tiles and singles of the grouped route) and W2's
        (gout)"""
        out = {}
        for kind in ("tile", "small", "single"):
            gs = [g for g in self.groups if g.kind == kind]
            if not gs:
                continue
            rows = np.concatenate([np.arange(g.row0, g.row0 + g.nrows) for g in gs])
            f1, o1, f3, o3, f2, o2 = [], [], [], [], [], []
            for g in gs:
                X, G1 = self.gin[g.row0:g.row0 + g.nrows], self.g1[g.row0:g.row0 + g.nrows]
                p1, p3 = self.pre64(kind, g.expert, 0, X), self.pre64(kind, g.expert, 1, X)
                y1, y3 = self.orc16(kind, g.expert, 0, X), self.orc16(kind, g.expert, 1, X)
                f1.append(self.glu64(p1, p3)); o1.append(o.mul(o.act(np.ascontiguousarray(y1), self.act), np.ascontiguousarray(y3)))
                f3.append(p3); o3.append(y3)
                f2.append(self.pre64(kind, g.expert, 2, G1)); o2.append(self.orc16(kind, g.expert, 2, G1))
            for name, f, r in (("g1", f1, o1), ("g3", f3, o3), ("gout", f2, o2)):
                if name == "g3" and not with_g3:
                    continue
                f64, orc = np.concatenate(f), np.concatenate(r).astype(np.float64)
                d_ref = float(np.abs(orc - f64).max())
                out["%ss.%s" % (kind, name)] = LaunchRef("%ss.%s" % (kind, name), rows, f64, orc, d_ref, np.maximum(2.0 * d_ref, ulp16(f64)))
        return out

    # -- faults: (name, launch name, float64 of the launch's rows with the fault) on this step's own lists
    def faults(self):
        gs = self.groups
        n = len(self.gin)
        by = {}
        for g in gs:
            by.setdefault(g.kind, []).append(g)

        def assemble(kind, name, fn):
            """fn(g) -> float64 rows of group g (None: as the correct launch)"""
            parts = []
            for g in by[kind]:
                v = fn(g)
                if v is None:
                    X = (self.gin if name != "gout" else self.g1)[g.row0:g.row0 + g.nrows]
                    v = self.glu64(self.pre64(kind, g.expert, 0, X), self.pre64(kind, g.expert, 1, X)) if name == "g1" else \
                        self.pre64(kind, g.expert, 2 if name == "gout" else 1, X)
                parts.append(v)
            return np.concatenate(parts)

        def g1_of(kind, e, X):
            return self.glu64(self.pre64(kind, e, 0, X), self.pre64(kind, e, 1, X))

        E = len(self.ex)
        for kind, lst in by.items():
            first = lst[0]
            # the neighbouring expert's weights
            yield "%s: a group computed with the neighbouring expert's weights" % kind, "%ss.g1" % kind, assemble(
                kind, "g1", lambda g: g1_of(kind, (g.expert + 1) % E, self.gin[g.row0:g.row0 + g.nrows]) if g is first else None)
            yield "%s: a group computed with the neighbouring expert's weights (W2)" % kind, "%ss.gout" % kind, assemble(
                kind, "gout", lambda g: self.pre64(kind, (g.expert + 1) % E, 2, self.g1[g.row0:g.row0 + g.nrows]) if g is first else None)
            # w1 / w3 exchanged in the table
            yield "%s: w1 / w3 table columns exchanged" % kind, "%ss.g1" % kind, assemble(
                kind, "g1", lambda g: self.glu64(self.pre64(kind, g.expert, 1, self.gin[g.row0:g.row0 + g.nrows]), self.pre64(kind, g.expert, 0, self.gin[g.row0:g.row0 + g.nrows])))
            if kind == "single":
                # pos taken as the list index
                moved = [(k, g) for k, g in enumerate(lst) if g.row0 != k and not np.array_equal(self.gin[k], self.gin[g.row0])]      # (the same token row at both places: nothing to see)
                if moved:
                    ks = dict((id(g), k) for k, g in moved)
                    yield "single: pos taken as its list index", "singles.g1", assemble(
                        kind, "g1", lambda g: g1_of(kind, g.expert, self.gin[ks[id(g)]:ks[id(g)] + 1]) if id(g) in ks else None)
                continue
            # row0 off by one (the row behind the last: the next entry, zeros behind the last entry)
            def shifted(A, g):
                X = np.zeros((g.nrows, A.shape[1]), np.float16)
                src = A[g.row0 + 1:g.row0 + 1 + g.nrows]
                X[:len(src)] = src
                return X
            yield "%s: row0 off by one" % kind, "%ss.g1" % kind, assemble(kind, "g1", lambda g: g1_of(kind, g.expert, shifted(self.gin, g)))
            yield "%s: row0 off by one (W2)" % kind, "%ss.gout" % kind, assemble(kind, "gout", lambda g: self.pre64(kind, g.expert, 2, shifted(self.g1, g)))
            # the last row of a group taken from the next group (its expert's weights)
            nxt = {id(g): gs[i + 1] for i, g in enumerate(gs[:-1])}
            have = [g for g in lst if id(g) in nxt]
            if have:
                def last_from_next(g):
                    if id(g) not in nxt:
                        return None
                    v = g1_of(kind, g.expert, self.gin[g.row0:g.row0 + g.nrows])
                    v[-1] = g1_of(kind, nxt[id(g)].expert, self.gin[g.row0 + g.nrows - 1:g.row0 + g.nrows])[0]
                    return v
                yield "%s: row nrows - 1 of a group taken from the next group" % kind, "%ss.g1" % kind, assemble(kind, "g1", last_from_next)
            if kind == "tile":
                # a partial tile read (and written) at full height: the rows behind it, other experts' rows, get this expert's product
                partial = [g for g in lst if g.nrows % 64 and g.row0 + g.nrows < n]
                if partial:
                    g0 = partial[0]
                    over = np.arange(g0.row0 + g0.nrows, min(n, g0.row0 + (64 if g0.nrows < 64 else 128)))
                    hit = {}
                    for kind2, lst2 in by.items():
                        rows2 = np.concatenate([np.arange(g.row0, g.row0 + g.nrows) for g in lst2])
                        m = np.isin(rows2, over)
                        if m.any():
                            f = self.launch_f64(kind2, "g1")
                            f[m] = g1_of("tile", g0.expert, self.gin[rows2[m]])
                            hit[kind2] = f
                    for kind2, f in hit.items():
                        yield "tile: a partial tile at full height (rows of the %ss overwritten)" % kind2, "%ss.g1" % kind2, f
            if kind == "small":
                # a 128-column superstep dropped from a group of <= 4 rows (staged whole): the last superstep of W2's K
                four = [g for g in lst if g.nrows <= 4]
                if four:
                    K = self.g1.shape[1]
                    def dropped(g):
                        if g.nrows > 4:
                            return None
                        X = self.g1[g.row0:g.row0 + g.nrows].astype(np.float64)
                        w = self.ex[g.expert].w64(2, "half")
                        return X @ w.T - X[:, K - 128:] @ w[:, K - 128:].T
                    if np.abs(self.g1[np.concatenate([np.arange(g.row0, g.row0 + g.nrows) for g in four])][:, K - 128:]).max() > 0:
                        yield "small: a 128-column superstep dropped from a whole-staged group", "smalls.gout", assemble(kind, "gout", dropped)

    def launch_f64(self, kind, name):
        gs = [g for g in self.groups if g.kind == kind]
        out = []
        for g in gs:
            X = (self.gin if name != "gout" else self.g1)[g.row0:g.row0 + g.nrows]
            out.append(self.glu64(self.pre64(kind, g.expert, 0, X), self.pre64(kind, g.expert, 1, X)) if name == "g1" else self.pre64(kind, g.expert, 2 if name == "gout" else 1, X))
        return np.concatenate(out)


FAULT_KINDS = ("a group computed with the neighbouring expert's weights", "w1 / w3 table columns exchanged", "row0 off by one",
               "row nrows - 1 of a group taken from the next group", "a partial tile at full height", "pos taken as its list index",
               "a 128-column superstep dropped from a whole-staged group")


def check_launch(out16, ref):
    """every element of the launch's rows within its bound of float64; returns (median, worst) err / bound"""
    a = np.asarray(out16).astype(np.float64)
    assert a.shape == ref.f64.shape, (ref.name, a.shape, ref.f64.shape)
    assert np.isfinite(a).all(), "%s: output is not finite" % ref.name
    r = np.abs(a - ref.f64) / ref.bound
    w = np.unravel_index(int(r.argmax()), r.shape)
    assert r[w] <= 1.0, "%s: entry %d column %d is %.3g from float64, bound %.3g (d_ref %.3g; %d of %d elements over)" % (
        ref.name, int(ref.rows[w[0]]), w[1], abs(a[w] - ref.f64[w]), ref.bound[w], ref.d_ref, int((r > 1.0).sum()), r.size)
    return float(np.median(r)), float(r[w])


def device_like(ref, f64_faulty=None):
    """the F16 rows a device would leave: the oracle's value, shifted by what a fault moves in float64"""
    if f64_faulty is None:
        return ref.orc.astype(np.float16)
    return (ref.orc + (f64_faulty - ref.f64)).astype(np.float16)


def host_step(rc, experts, seed=0):
    """the inputs of a step as the host test makes them: the oracle's normalised rows gathered, g1 by the oracle per group"""
    r = host_router(rc)
    L = M.build_lists(r["sel"], r["w"], rc.n, rc.K, rc.E, expected_plan(rc)["tile_rows"], expected_plan(rc)["small_max"])
    gin = r["hn"][L.idx]
    ref = LayerRef(experts, L, gin, np.zeros((len(gin), rc.ffn), np.float16))
    g1 = np.zeros((len(gin), rc.ffn), np.float16)
    for g in ref.groups:
        X = gin[g.row0:g.row0 + g.nrows]
        g1[g.row0:g.row0 + g.nrows] = o.mul(o.act(np.ascontiguousarray(ref.orc16(g.kind, g.expert, 0, X)), 0), np.ascontiguousarray(ref.orc16(g.kind, g.expert, 1, X)))
    return LayerRef(experts, L, gin, g1), r

