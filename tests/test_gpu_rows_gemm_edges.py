"""-m gpu: every launch of the rows GEMM (k_gemm_rows_mfma: QKV, Wo, W1 / W3, W2 of a batched decode step and of a 2..32-token prompt) against
the oracle's arithmetic and plain float64 math, each launch from the inputs the DEVICE had, at the row, tile, chunk and K-part counts where the
launcher changes instance.  tests/rows_gemm_util.py has the cases, the reference and the assertions; tests/test_rows_gemm_ref_cpu.py shows on
the host that those assertions reject every fault of docs/rows_gemm_edges.md for every launch shape walked here.

One case: a one-layer model (weights N(0, 0.055) quantised on the device, rope_order 0, 32 F16 embedding rows = the layer inputs: token i
selects row i, 32 KV slots, 4 context rows).  A step of n rows runs eagerly (logits requested) at position 0 of n slots.  Before any number
is compared the batched step's route plan must be the fused one and the four launch records (ifa_gemm_rows_launches) must equal the first
attempt of ifa_gemm_rows_plan for that launch on THIS device; then
  QKV    bqkv = (Wq | Wk | Wv) . norm(E)          norm-fused (or behind the norm launch, whose output the step overwrites): exact on the sign family
  Wo     a    = E + Wo . att + b                  att: the attention's own output, read back                                 exact
  W1/W3  t1   = act(W1 . h) x (W3 . h)            h = norm(a) fused (flip term), or the norm launch's output read back (exact)
  W2     x'   = a + W2 . t1 + b                   t1: the device's own                                                      exact
The rows of x, att, a and t1 past row n must keep what they held (a sentinel pattern after the first, largest step), the embedding rows and
every weight tensor must be byte-identical after a model's steps, and no wait error may be reported (decode_batch fails on one)."""
import os

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth, worker as W
from tests import prompt_gemm_util as P
from tests import rows_gemm_util as U

pytestmark = pytest.mark.gpu
V = 32
MATS = ((W.T_WQ, W.T_WQ_B, "wq"), (W.T_WK, W.T_WK_B, "wk"), (W.T_WV, W.T_WV_B, "wv"), (W.T_WO, W.T_WO_B, "wo"), (W.T_W1, W.T_W1_B, "w1"),
        (W.T_W3, W.T_W3_B, "w3"), (W.T_W2, W.T_W2_B, "w2"))
B_FACTS = ("n", "exact_order", "may_chunk", "rows_mo", "gemm_rows", "batch_fused", "rows_kparts", "batch_graph", "graph", "topo", "rows_layers",
           "has_moe", "logits_out")
B_OUT = ("kind", "chunk", "norm_fused", "captured", "gm_kernel", "gm_src", "gm_mo", "gm_no_waits", "need_mo")


def _cus():
    import ctypes as C
    n = torch.cuda.get_device_properties(0).multi_processor_count
    vis = n
    if os.environ.get("IFA_VISIBLE_CUS"):
        vis = min(n, int(os.environ["IFA_VISIBLE_CUS"]))
    else:
        for name in ("ROC_GLOBAL_CU_MASK", "HSA_CU_MASK"):
            if os.environ.get(name):
                vis = ia.lib().ifa_visible_cus_from_mask(os.environ[name].encode(), 0, vis)
    return n, vis


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float16).view(np.int16)).to("cuda:0").view(torch.float16)


def _embeddings(mc):
    return U.make_rows(mc.family, V, mc.dim, 4000 + mc.dim + 7 * mc.qd + 3 * mc.ffn, U.tail_cols(mc.dim))


def _build(mc, E, max_ctx=4):
    s = dict(dim=mc.dim, layers=1, heads=mc.heads, kv_heads=mc.kv_heads, head_dim=mc.head_dim, ffn=mc.ffn, vocab=V)
    wk = W.DecodeWorker(max_ctx=max_ctx, kv_dtype=dt.F16, rope_order=0, **s)
    dev = "cuda:0"
    wk.set_tensor_f16(-1, W.T_EMBD, dt.F16, _dev16(E))
    wk.set_tensor_f16(-1, W.T_OUT_NORM, dt.F16, torch.ones(mc.dim, dtype=torch.float16, device=dev))
    wk.set_tensor_f16(-1, W.T_LM_HEAD, dt.F16, synth.gen_f16((V, mc.dim), 998, U.W_STD, dev))
    nw = _dev16(U.norm_weight(mc.dim))
    wk.set_tensor_f16(0, W.T_ATTN_NORM, dt.F16, nw)
    wk.set_tensor_f16(0, W.T_FFN_NORM, dt.F16, nw)
    bias = {t: b for t, b, _ in MATS}
    for tid, kind in synth.MATRICES:
        rows, cols = synth._shape(kind, s)
        t16 = synth.gen_f16((rows, cols), 1000 + tid, U.W_STD, dev)
        if mc.family == "tail" and tid in (W.T_WV, W.T_W1, W.T_W3):      # att (= v at position 0) and t1 become tail-only
            t16[:U.tail_cols(rows)[0]] = 0
        wk.set_tensor_f16(0, tid, mc.wd, t16, rows, cols)
        if mc.bias:
            wk.set_tensor_f16(0, bias[tid], dt.F16, synth.gen_f16((rows,), 2000 + tid, U.B_STD, dev))
    wk.finalize()
    wk.kv_slots(V)
    wk.set_option("rows_mo", mc.mo)
    wk.set_option("rows_kparts", mc.kparts)
    return wk


def _tensors(wk):
    ids = [t for t, _, _ in MATS] + [b for _, b, _ in MATS]
    out = {tid: wk.get_tensor_host(0, tid) for tid in ids}
    out[W.T_EMBD] = wk.get_tensor_host(-1, W.T_EMBD)
    return out


def _same_tensors(wk, raw, where):
    now = _tensors(wk)
    for tid, v in raw.items():
        assert (v is None) == (now[tid] is None) and (v is None or np.array_equal(v[1], now[tid][1])), ("a tensor changed", where, tid)


def _mats(raw):
    m = {}
    for tid, btid, name in MATS:
        d, data, rows, cols = raw[tid]
        m[name] = P.Mat(d, data, rows, cols, bias=raw[btid][1].view(np.float16) if raw[btid] is not None else None)
    return m


def _route(mc, n):
    import ctypes as C
    f = dict(n=n, exact_order=0, may_chunk=1, rows_mo=mc.mo, gemm_rows=1, batch_fused=1, rows_kparts=mc.kparts, batch_graph=0, graph=1, topo=0,
             rows_layers=2 if mc.wd in (dt.Q4_B32T1A, dt.Q4_B32T1B) else 1, has_moe=0, logits_out=1)
    facts = (C.c_int * len(B_FACTS))(*[int(f[k]) for k in B_FACTS])
    out = (C.c_int * len(B_OUT))()
    ia.check(ia.lib().ifa_batch_route_plan(facts, len(B_FACTS), out, len(B_OUT)))
    return dict(zip(B_OUT, out))


def _assert_records(mc, n, recs, total, where):
    """the four launches of the step are the first attempts of their plans on this device"""
    num_cus, vis = _cus()
    assert total == 4 and len(recs) == 4, (where, "launches recorded", total)
    plans = {}
    for role, rec in zip(U.ROLES, recs):
        c = mc.launches(n)[role]
        p = plans[role] = c.plan(num_cus, vis, no_waits=0 if mc.kparts else 1)
        assert p["error"] == 0, (where, role, p)
        t = p["tries"][0]
        want = dict(T=n, total_rows=c.N, nblk=c.K // 32, epi=c.epi, norm=c.norm, mo=mc.mo, tx=p["tx"], ch=p["ch"], nchunk=p["nchunk"], n_try=len(p["tries"]),
                    attempt=0, **t)
        diff = {k: (rec[k], v) for k, v in want.items() if rec[k] != v}
        assert not diff, "%s %s: the launch that ran differs from the plan's first attempt, (ran, planned) = %s; the whole record: %s" % (where, role, diff, rec)
        if not mc.kparts:
            assert t["kparts"] == 0, (where, role, "rows_kparts 0 must run the plain attempt")
    return plans


class Stats:
    def __init__(self, title):
        self.title, self.rows, self.failed = title, {}, []

    def add(self, role, where, out16, ref):
        try:
            med, worst, share, need = U.check(out16, ref)
        except AssertionError as e:                      # (every launch of the walk is measured before the test fails)
            need = U.flips_needed(out16, ref)
            self.failed.append("%s %s: %s [flips needed: most %d, %d elements > 0]" % (where, role, e, int(need.max()), int((need > 0).sum())))
            return
        self.rows.setdefault(role, []).append((worst, med, share, need, where, ref.exact))

    def report(self):
        for role, v in self.rows.items():
            w = max(v)
            pro = [x for x in v if not x[5]]
            print("rows-gemm-edges %-44s %-4s %3d launches  median %.3f  worst err / bound %.3f (%s)%s" % (
                self.title, role, len(v), float(np.median([x[1] for x in v])), w[0], w[4],
                "  flip-term launches %d: most elements on it %.2f %%, most flips %d" % (len(pro), 100 * max(x[2] for x in pro), max(x[3] for x in pro)) if pro else ""))
        assert not self.failed, "%d launches of %s: %s" % (len(self.failed), self.title, " | ".join(self.failed))


class Tracker:
    """what the row buffers must hold outside the rows a step writes: a host copy per buffer (x: one per physical buffer -- a one-layer step
    gathers into one and leaves its output in the other, which is the one "rows_x" shows afterwards)"""

    def __init__(self, wk, rows):
        self.wk, self.R = wk, rows
        self.held = {}
        self.x = [None, None]
        self.vis = 0

    def sentinel(self, name):
        p, n = self.wk.buffer(name)
        cols = n // 2 // self.R
        s = P.sentinel_frame(self.R - P.PAD_ROWS, cols, cols)
        self.wk.write_buffer(name, s)
        return s

    def after_step(self, n, E, where):
        """reads x (the step's output), att, a, t1; checks the rows past n; returns the first n rows of each"""
        out = {}
        hidden = 1 - self.vis                                    # the gather wrote E[:n] into the visible buffer, the output went to the other
        if self.x[self.vis] is not None:
            self.x[self.vis][:n] = E[:n].view(np.uint16)
        self.vis = hidden
        for name in ("rows_x", "rows_att", "rows_a", "rows_t1"):
            got = self.wk.read_buffer(name).view(np.uint16).reshape(self.R, -1)
            was = self.x[self.vis] if name == "rows_x" else self.held.get(name)
            if was is not None:
                assert np.array_equal(got[n:], was[n:]), "%s: rows of %s past row %d changed (first at row %d)" % (
                    where, name, n, n + int(np.argwhere((got[n:] != was[n:]).any(axis=1))[0]))
            out[name] = got[:n].copy().view(np.float16)
            fresh = self.sentinel(name) if was is None else None      # (first sight of this buffer: every row becomes the pattern)
            keep = fresh if fresh is not None else got
            if name == "rows_x":
                self.x[self.vis] = keep.copy()
            else:
                self.held[name] = keep.copy()
        return out


def _step(wk, mc, mats, E, nw, n, tr, stats, where, check=True):
    W.gemm_rows_launches()
    lg = torch.empty((n, V), dtype=torch.float16, device="cuda:0")
    wk.decode_batch(np.arange(n), np.zeros(n), np.arange(n), lg)
    recs, total = W.gemm_rows_launches()
    r = _route(mc, n)
    assert (r["kind"], r["norm_fused"], r["captured"], r["gm_kernel"], r["gm_mo"], r["gm_no_waits"]) == (2, int(mc.norm_fused(n)), 0, 0, mc.mo, int(not mc.kparts)), (where, r)
    plans = _assert_records(mc, n, recs, total, where)
    bufs = tr.after_step(n, E, where)
    bqkv = wk.read_buffer("rows_bqkv").view(np.float16).reshape(32, -1)[:n]
    if not check:
        return bufs, bqkv, plans
    cs = mc.launches(n)
    att, a, t1, xo = bufs["rows_att"], bufs["rows_a"], bufs["rows_t1"], bufs["rows_x"]
    En = E[:n]
    if mc.family == "tail":
        for name, v in (("att", att), ("t1", t1)):
            lo = U.tail_cols(v.shape[1])[0]
            assert not v[:, :lo].any() and v[:, lo:].any(), ("the tail-only input of the plain launches is not tail-only", where, name)
    refs = {}
    qm = [mats["wq"], mats["wk"], mats["wv"]]
    refs["qkv"] = (U.RowsRef(U.RInputs(cs["qkv"], qm, None, U.normed(En, nw), raw=En, norm_w=nw)), bqkv)
    refs["wo"] = (U.RowsRef(U.RInputs(cs["wo"], [mats["wo"]], None, att, res=En)), a)
    if cs["w13"].norm:
        i13 = U.RInputs(cs["w13"], [mats["w1"]], mats["w3"], U.normed(a, nw), raw=a, norm_w=nw)
    else:
        hn = wk.read_buffer("rows_hn").view(np.float16).reshape(tr.R, -1)[:n]
        i13 = U.RInputs(cs["w13"], [mats["w1"]], mats["w3"], hn)
    refs["w13"] = (U.RowsRef(i13), t1)
    refs["w2"] = (U.RowsRef(U.RInputs(cs["w2"], [mats["w2"]], None, t1, res=a)), xo)
    for role in U.ROLES:
        stats.add(role, where, refs[role][1], refs[role][0])
    return bufs, bqkv, plans


def _walk(mc, stats):
    E = _embeddings(mc)
    wk = _build(mc, E)
    raw = _tensors(wk)
    assert np.array_equal(raw[W.T_EMBD][1].view(np.uint16).reshape(V, -1), E.view(np.uint16))
    mats = _mats(raw)
    nw = U.norm_weight(mc.dim)
    tr = Tracker(wk, mc.ns[0])
    first = None
    for i, n in enumerate(mc.ns + mc.ns[:1]):              # (the largest first -- it sizes the buffers -- and once more at the end: both x buffers seen)
        bufs, bqkv, _ = _step(wk, mc, mats, E, nw, n, tr, stats, "%s n=%d" % (mc.id, n), check=i < len(mc.ns))
        if i == 0:
            first = dict(bufs, rows_bqkv=bqkv.copy())
    # the copies of the weights the kernels read (tiled, MO) have no view: after every step of the model the first step, run again, must
    # give the bytes it gave at first -- the copies, the norm weights and the biases still produce the same numbers
    for name, v in dict(bufs, rows_bqkv=bqkv).items():
        assert np.array_equal(v.view(np.uint16), first[name].view(np.uint16)), "%s: %s of the first step, run again after all the others, differs" % (mc.id, name)
    _same_tensors(wk, raw, mc.id)
    return wk


CASES = U.model_cases(torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256)


@pytest.mark.parametrize("mc", CASES, ids=[c.id for c in CASES])
def test_every_launch_of_a_batched_step(mc):
    stats = Stats(mc.id)
    wk = _walk(mc, stats)
    wk.close()
    stats.report()


# ----------------------------------------------------------------------------- K parts: repeatable, and the same under capture
def _kparts_model():
    return U.ModelCase("kparts", dt.Q4_B32T1A, 1, 128, 64, 64, 128, 12288, (16,), bias=True)


def _read_all(wk, mc, n):
    """the first n rows of the step's outputs (the rows past them are not the step's: a fresh buffer holds whatever the allocator left)"""
    width = dict(rows_x=mc.dim, rows_att=mc.qd, rows_a=mc.dim, rows_t1=mc.ffn, rows_bqkv=mc.qd + 2 * mc.kvd)
    return {name: wk.read_buffer(name).view(np.uint16).reshape(-1, w)[:n].copy() for name, w in width.items()}


def test_kparts_step_is_bit_identical_three_times_and_under_capture():
    """Wo (K 8192: 2 parts) and W2 (K 12288: 3 parts) of one step take K parts with different group counts.  Four eager runs, a fifth behind
    a 32-row step with other part counts, a captured and a replayed run leave the same bytes in every row buffer, W2's output included:
    the granules are zero again after every launch, whatever ran before (a granule left behind would be added to the next launch's sum)"""
    mc = _kparts_model()
    E = _embeddings(mc)
    wk = _build(mc, E)
    n = 16
    tok, pos, sl = np.arange(n), np.zeros(n), np.arange(n)
    lg = torch.empty((n, V), dtype=torch.float16, device="cuda:0")
    W.gemm_rows_launches()
    runs = []
    for i in range(4):                                       # (x and its twin alternate: runs 0 and 2, 1 and 3 share a buffer; all must agree)
        wk.decode_batch(tok, pos, sl, lg)
        runs.append(_read_all(wk, mc, n))
    recs, total = W.gemm_rows_launches()
    assert total == 16
    parts = [r["kparts"] for r in recs[-4:]]
    p_wo, p_w2 = (mc.launches(n)[r].plan(*_cus()) for r in ("wo", "w2"))
    assert parts == [0, p_wo["tries"][0]["kparts"], 0, p_w2["tries"][0]["kparts"]] and parts[1] >= 2 and parts[3] >= 2 and parts[1] != parts[3], (parts, recs[-4:])
    assert p_wo["tries"][0]["groups"] != p_w2["tries"][0]["groups"]
    # a step of another row count (other part counts, groups and granule slots: 17..32 rows stage 2048-column chunks), then this one again
    n2 = 32
    lg2 = torch.empty((n2, V), dtype=torch.float16, device="cuda:0")
    wk.decode_batch(np.arange(n2), np.zeros(n2), np.arange(n2), lg2)
    recs, total = W.gemm_rows_launches()
    assert total == 4 and [r["kparts"] >= 2 for r in recs] == [False, True, False, True] and [r["kparts"] for r in recs] != parts, recs
    wk.decode_batch(tok, pos, sl, lg)
    runs.append(_read_all(wk, mc, n))
    W.gemm_rows_launches()
    for r in runs[1:]:
        for name in r:
            assert np.array_equal(r[name], runs[0][name]), name
    first = wk.decode_batch(tok, pos, sl)                    # no logits requested: captured, run once
    cap = _read_all(wk, mc, n)
    again = wk.decode_batch(tok, pos, sl)                    # replayed
    rep = _read_all(wk, mc, n)
    recs, total = W.gemm_rows_launches()
    assert total == 4, "the capture records its four launches, the replay none"
    assert list(first) == list(again)
    for name in cap:                                         # (rows_x too: the capture swaps x and its twin on the host, the replay writes the same addresses)
        assert np.array_equal(cap[name], runs[0][name]) and np.array_equal(rep[name], runs[0][name]), name
    wk.close()


# ----------------------------------------------------------------------------- the two layouts agree bit for bit
@pytest.mark.parametrize("n", (2, 3, 4, 5, 8))
def test_mo_layout_equals_the_tiled_layout_bit_for_bit(n):
    """csrc/ifa_gemm_rows_mfma_body.h: same operands, same MFMA order -- up to 8 rows both layouts stage 4096-column chunks"""
    outs = []
    for mo in (1, 0):
        mc = U.ModelCase("rows", dt.Q4_B32T1A, mo, 256, 8, 8, 32, 4352, (n,), bias=True)
        wk = _build(mc, _embeddings(mc))
        lg = torch.empty((n, V), dtype=torch.float16, device="cuda:0")
        wk.decode_batch(np.arange(n), np.zeros(n), np.arange(n), lg)
        outs.append(_read_all(wk, mc, n))
        wk.close()
    for name in outs[0]:
        assert np.array_equal(outs[0][name], outs[1][name]), name


# ----------------------------------------------------------------------------- the prompt route
PROMPTS = [(mo, T) for mo in (1, 0) for T in U.PROMPT_TOKENS if mo or T <= 16]      # (the tiled layout serves up to 16 rows)


@pytest.mark.parametrize("mo,T", PROMPTS, ids=["%s-T%d" % ("mo" if m else "tiled", t) for m, t in PROMPTS])
def test_every_launch_of_a_short_prompt(mo, T):
    """forward() of T tokens (40: 32 + 8, two passes): q, k, v as three matrices (Yset), a, t1 and the output rows, each from the inputs the
    device had"""
    mc = U.prompt_model(mo)
    E = _embeddings(mc)
    wk = _build(mc, E, max_ctx=64)
    mats = _mats(_tensors(wk))
    nw = U.norm_weight(mc.dim)
    stats = Stats("prompt %s T=%d" % ("mo" if mo else "tiled", T))
    passes = U.prompt_passes(T)
    toks = np.arange(T) % V
    if T == 40:
        wk.set_option("prefill_mid", 0)                      # (k_gemm_mid would take 33..48 tokens in one pass: the two passes are the route without it)
    W.gemm_rows_launches()
    wk.forward(toks, 0)
    route = wk.prompt_route()
    recs, total = W.gemm_rows_launches()
    assert route["kind"] == "rows" and route["first_pass"] == (32 if T == 40 else 0), route
    assert total == 4 * len(passes), total
    # only the LAST pass's buffers survive: it is the one compared
    t0, n = passes[-1]
    recs = recs[-4:]
    num_cus, vis = _cus()
    width = dict(rows_q=mc.qd, rows_k=mc.kvd, rows_v=mc.kvd, rows_att=mc.qd, rows_a=mc.dim, rows_t1=mc.ffn, rows_x=mc.dim, rows_hn=mc.dim)
    rd = lambda name: wk.read_buffer(name).view(np.float16).reshape(-1, width[name])[:n]
    En = E[toks[t0:t0 + n]]
    cs = mc.launches(n)
    nf = int(mc.norm_fused(n))
    for role, rec in zip(U.ROLES, recs):
        p = cs[role].plan(num_cus, vis)
        want = dict(T=n, total_rows=cs[role].N, nblk=cs[role].K // 32, epi=cs[role].epi, norm=cs[role].norm, mo=mo, tx=p["tx"], ch=p["ch"], attempt=0, **p["tries"][0])
        diff = {k: (rec[k], v) for k, v in want.items() if rec[k] != v}
        assert not diff, (role, diff, rec)
    q, k, v, att, a, t1, xo = (rd(x) for x in ("rows_q", "rows_k", "rows_v", "rows_att", "rows_a", "rows_t1", "rows_x"))
    qkv = np.concatenate([q, k, v], axis=1)
    where = "T=%d" % T
    stats.add("qkv", where, qkv, U.RowsRef(U.RInputs(cs["qkv"], [mats["wq"], mats["wk"], mats["wv"]], None, U.normed(En, nw), raw=En, norm_w=nw)))
    stats.add("wo", where, a, U.RowsRef(U.RInputs(cs["wo"], [mats["wo"]], None, att, res=En)))
    if nf:
        i13 = U.RInputs(cs["w13"], [mats["w1"]], mats["w3"], U.normed(a, nw), raw=a, norm_w=nw)
    else:
        i13 = U.RInputs(cs["w13"], [mats["w1"]], mats["w3"], rd("rows_hn"))
    stats.add("w13", where, t1, U.RowsRef(i13))
    stats.add("w2", where, xo, U.RowsRef(U.RInputs(cs["w2"], [mats["w2"]], None, t1, res=a)))
    wk.close()
    stats.report()
