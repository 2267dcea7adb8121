"""-m gpu: every fused GEMV launch of the decode step itself (k_dec_gemv, k_dec_gemv_long, k_dec_gemv_h: QKV, Wo, W1 / W3, W2) against the
oracle's arithmetic and plain float64 math, each launch from the inputs the DEVICE had, at the column and row counts where the launcher
changes instance.  tests/decode_gemv_util.py has the reference, the inputs and the assertions; tests/test_decode_gemv_ref_cpu.py shows
on the host that those assertions reject a lost, doubled or mis-paired block, a missing zero-point term, a lost or doubled residual and a
row finished with another row's sum, for every format and width walked here.  docs/decode_gemv_edges.md has the instance table and the
measured figures.

One case: a one-layer model (weights N(0, 0.06), vocabulary 64, 8 context rows, options fuse_attn 0, fuse_ffn 0, step_tail 0 -- the
step's last launch would otherwise gather the next token into "x" --, debug_hidden_in 1); the test writes the layer input "x", one step
runs at position 0, and "dqkv", "att", "attq", "a", "t1", "x2" are read back.  Before any number is compared the plan of each
launch (Worker.gemv_plan) must show the kernel, nj, nchunk and npass the case claims, and that the step runs the launch on its own; grid,
waves, npass and partial are recomputed here from the plan's rw / threads and the CU count of the device the test runs on.
  QKV    dqkv  = (Wq | Wk | Wv) . Q8(norm(x))                                   prologue launch
  Wo     a     = x + s_a (Wo . attq + b)       attq: the attention's own Q8 image, read back (Q8(att) where the launch quantises)   exact
  W1/W3  t1    = act(W1 . Q8(norm(a))) x (W3 . Q8(norm(a)))                     prologue launch
  W2     x2    = a + s_f (W2 . Q8(t1) + b)     t1: the device's own                                                            exact
Exact launches: every element within max(2 x d_ref, one F16 ulp at |out|) of float64 (d_ref = max|oracle - float64| of the launch).
Prologue launches are exact too on the sign family (+-1: the normalised vector is +-1 whatever the last bit of the norm); on dense and
tail-only inputs a row may use F = 1 flip of one Q8 code (max|w of the row| x max block scale each) on top, and at most 2 % of a launch's
rows may need that term (printed per launch).  F is the worst count measured on MI355X plus one (docs/decode_gemv_edges.md).

Model families (no matrix larger than 32768 x 256):
  wide    dim = c, 4 heads of 32, ffn 256: QKV and W1 / W3 see c columns.  attn_out_scale = 1e-12 turns Wo's product into 0 before the
          residual is added, so a == x bit for bit and W1 / W3 see the same controlled input as QKV (the buffer "a" cannot be written: the
          step recomputes it).
  long    dim 256, c / 32 heads of 32 (dim != heads x head_dim), ffn = c: Wo and W2 see c columns, W1 / W3 have c row pairs.  "tail": the
          rows of Wv, W1 and W3 in front of the last round of blocks are zero, so att (= the step's own v at position 0) and t1 are
          zero there: the tail-only input of Wo and W2.
Seeds of the layer input: 1000 + c where QKV and W1 / W3 see c columns, 3000 for the long models' 256 values (U.seed_of, U.SEED_LONG);
tests/test_decode_gemv_ref_cpu.py proves the sensitivity of the assertions at these widths and seeds.
What cannot be built: fewer W1 / W3 rows than one workgroup has waves (ffn must be a multiple of 32, and of W2's block size: t1 is
quantised in blocks of 32 and read in whole weight blocks), so the smallest launch has 32 or 64 row pairs; no format reaches 4 chunks
below 32768 columns and only Q8_B32T2 reaches 3 (tests/test_decode_gemv_plan_cpu.py).

Measured on MI355X (256 CUs; the whole file: 54 ids in 38 s), err = |out - float64| / bound per launch, the bound being 1; 0.500 means
the worst row is the oracle's value bit for bit (its distance from float64 is d_ref itself).  Worst over the launches of a family:
  wide, int8-path formats (201 launches per role)     0.500; medians QKV 0.053, W1 / W3 0.004, W2 0.035 (Wo 0.000: its product is scaled to 0)
  long, int8-path formats (280 per role)              0.966 (Q4_B64T1 W1 / W3, 8192 row pairs, tail model), else 0.500; medians QKV 0.045, Wo 0.052, W2 0.063
  fp16-activation formats (162 per role)              0.538 (Q8_B32T1 Wo, 32768 columns), 0.514 (Q2_B32T1B W2, 2048 columns), else 0.500
  rows (18 per role)                                  0.500
  wirings (180 per role)                              0.500
Flips: no row of any prologue launch (dense and tail-only inputs; 1332 launches) was outside the exact bound -- 0.00 % of the rows on
the flip term, 0 flips needed, for every format and role -- so F = 0 + 1.

Remaining gaps: the MoE epilogues, the x_add (tensor-parallel seam) instances (the batched rows GEMM: tests/test_gpu_rows_gemm_edges.py); the chained and fused-tail launches
have their own bit-identity tests against these single launches (tests/test_gpu_chain.py, tests/test_gpu_fused_attn.py)."""
import numpy as np
import pytest

from inferflow_amd import dtypes as dt, synth, worker as W
from tests import decode_gemv_util as U

pytestmark = pytest.mark.gpu
F = 1
TOK = 5
STD = 0.06
BIAS = ((W.T_WQ, W.T_WQ_B), (W.T_WK, W.T_WK_B), (W.T_WV, W.T_WV_B), (W.T_WO, W.T_WO_B), (W.T_W1, W.T_W1_B), (W.T_W3, W.T_W3_B), (W.T_W2, W.T_W2_B))
NAMES = {W.T_WQ: "wq", W.T_WK: "wk", W.T_WV: "wv", W.T_WO: "wo", W.T_W1: "w1", W.T_W3: "w3", W.T_W2: "w2"}
ID = {d: dt.name(d).lower() for d in U.INT8_FORMATS + U.F16X_FORMATS}


def _build(wd, dim, heads, ffn, bias=False, zero_before=None, native=False, **cfg):
    """a one-layer model of 32-wide heads with every matrix in format wd; zero_before: {tensor id: rows in front of this one are zero}"""
    import torch
    s = dict(dim=dim, layers=1, heads=heads, kv_heads=heads, head_dim=32, ffn=ffn, vocab=64)
    wk = W.DecodeWorker(max_ctx=8, kv_dtype=dt.F16, **s, **cfg)
    dev = "cuda:0"
    ones = torch.ones(dim, dtype=torch.float16, device=dev)
    wk.set_tensor_f16(-1, W.T_EMBD, dt.F16, synth.gen_f16((64, dim), 999, STD, dev))
    wk.set_tensor_f16(-1, W.T_OUT_NORM, dt.F16, ones)
    wk.set_tensor_f16(-1, W.T_LM_HEAD, dt.F16, synth.gen_f16((64, dim), 998, STD, dev))
    full = dict(s, **cfg)
    if cfg.get("norm_kind"):                               # the std norm: weights and a bias (U.std_norm_affine says why)
        w, b = (torch.from_numpy(a.view(np.int16)).to(dev).view(torch.float16) for a in U.std_norm_affine(dim))
        for tid, t in ((W.T_ATTN_NORM, w), (W.T_ATTN_NORM_B, b), (W.T_FFN_NORM, w), (W.T_FFN_NORM_B, b)):
            wk.set_tensor_f16(0, tid, dt.F16, t)
    else:
        wk.set_tensor_f16(0, W.T_ATTN_NORM, dt.F16, ones)
        if not cfg.get("parallel_attn"):
            wk.set_tensor_f16(0, W.T_FFN_NORM, dt.F16, ones)
    for tid, kind in synth.MATRICES:
        if tid == W.T_W3 and not cfg.get("is_glu", 1):
            continue
        rows, cols = synth._shape(kind, s)
        t16 = synth.gen_f16((rows, cols), 1000 + tid, STD, dev)
        if zero_before and tid in zero_before:
            t16[:zero_before[tid]] = 0
        wk.set_tensor_f16(0, tid, wd, t16, rows, cols)
        if bias:
            wk.set_tensor_f16(0, dict(BIAS)[tid], dt.F16, synth.gen_f16((rows,), 2000 + tid, STD, dev))
    wk.finalize()
    ok, why = wk.fused_supported()
    assert ok, why                                         # (otherwise decode() would run the op-by-op step: other kernels)
    for k, v in (("fuse_attn", 0), ("fuse_ffn", 0), ("step_tail", 0), ("debug_hidden_in", 1), ("q3h_native", int(native))):
        wk.set_option(k, v)
    return wk, full


def _weights(wk):
    return {tid: wk.get_tensor_host(0, tid) for tid in list(NAMES) + [b for _, b in BIAS]}


def _model(wk, cfg, raw):
    mats = {}
    for tid, btid in BIAS:
        if raw[tid] is None:
            continue
        d, data, rows, cols = raw[tid]
        b = raw[btid][1].view(np.float16) if raw[btid] is not None else None
        mats[NAMES[tid]] = U.Mat(d, data, rows, cols, bias=b)
    ones = np.ones(cfg["dim"], np.float16)
    if cfg.get("norm_kind"):
        w, b = U.std_norm_affine(cfg["dim"])
        return U.Model(cfg, mats, dict(attn_norm=w, attn_norm_b=b, ffn_norm=w, ffn_norm_b=b))
    return U.Model(cfg, mats, dict(attn_norm=ones, ffn_norm=None if cfg.get("parallel_attn") else ones))


class Stats:
    """per launch role: (err / bound, share of rows on the flip term, flips needed) of every case; failures collected, reported at the end"""

    def __init__(self, title):
        self.title, self.rows, self.failed, self.cases = title, {}, [], 0

    def add(self, role, where, out16, launch):
        try:
            med, worst, share, need = U.check(out16, launch, F)
        except AssertionError as e:                      # (every case of the walk is measured before the test fails)
            need = U.flips_needed(out16, launch)
            self.failed.append("%s %s: %s [flips needed: worst row %d, %d rows > 0]" % (where, role, e, int(need.max()), int((need > 0).sum())))
            return
        self.rows.setdefault(role, []).append((worst, med, share, need, where, launch.exact))

    def report(self):
        for role, v in self.rows.items():
            w = max(v)
            pro = [x for x in v if not x[5]]
            print("decode-gemv-edges %-34s %-5s %3d launches  median %.3f  worst err / bound %.3f (%s)%s" % (
                self.title, role, len(v), float(np.median([x[1] for x in v])), w[0], w[4],
                "  prologue: %d launches, most rows on the flip term %.2f %%, most flips %d" % (len(pro), 100 * max(x[2] for x in pro), max(x[3] for x in pro)) if pro else ""))
        assert not self.failed, "%d launches of %s: %s" % (len(self.failed), self.title, " | ".join(self.failed))


def _assert_plan(wk, role, where, **want):
    got = wk.gemv_plan(0, role)
    want = dict(dict(single=1, error=0, launches=1), **want)
    # passes from the plan's own rw / threads and THIS device's CUs: W = grid x waves per workgroup, ceil(rows / (rw x W)) passes
    wpw = got["threads"] // 64
    grid = max(1, min(got["num_cus"] * (2 if got["kind"] == "f16x" else 1), -(-got["total_rows"] // (wpw * (got["rw"] if got["kind"] == "f16x" else 1)))))
    npass = -(-got["total_rows"] // (got["rw"] * grid * wpw))
    want.update(grid=grid, waves=grid * wpw, npass=want.get("npass", npass), partial=int(npass * got["rw"] * grid * wpw != got["total_rows"]))
    assert want["npass"] == npass, "%s %s: the case claims %d passes, %d rows on %d waves of %d rows make %d" % (where, role, want["npass"], got["total_rows"], grid * wpw, got["rw"], npass)
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not diff, "%s %s: planned launch differs from the case's, (got, want) = %s; the whole plan: %s" % (where, role, diff, got)
    return got


def _step(wk, cfg, model, x16, family, stats, where, roles=("qkv", "wo", "ffn13", "w2")):
    """x16 -> "x", one step at position 0, the launches named in roles against their references"""
    wk.write_buffer("x", x16.view(np.uint16))
    wk.decode(TOK, 0, 1)
    bufs = {n: wk.read_buffer(n).copy() for n in ("x", "dqkv", "att", "attq", "a", "t1", "x2") if wk.buffer(n)[1] > 0}
    assert np.array_equal(bufs["x"].view(np.uint16), x16.view(np.uint16)), ("the layer input changed", where)
    preq = wk.gemv_plan(0, "wo")["norm"] == 2
    launches, xn = U.step_launches(model, x16, bufs, family, preq)
    outs = dict(qkv="dqkv", wo="a", ffn13="t1", w2="x2")
    for role in roles:
        stats.add(role, where, bufs[outs[role]].view(np.float16), launches[role])
    return bufs, xn


def _same_weights(wk, raw, where):
    now = _weights(wk)
    for tid, v in raw.items():
        assert (v is None) == (now[tid] is None) and (v is None or np.array_equal(v[1], now[tid][1])), ("a weight tensor changed", where, tid)


# ----------------------------------------------------------------------------- columns of the normalised / gated inputs
WIDE = [(d, False) for d in U.INT8_FORMATS] + [(dt.Q3H_B64T1, True)]


def _wide_walk(wd, native, edges, stats, families=("dense", "sign", "tail"), kind="classic", heads=4, plan_dtype=None):
    for cols, nj in edges:
        wk, cfg = _build(wd, cols, heads, 256, native=native, attn_out_scale=1e-12)
        raw = _weights(wk)
        model = _model(wk, cfg, raw)
        for fam in families:
            where = "%d columns %s" % (cols, fam)
            bufs, _ = _step(wk, cfg, model, U.make_input(fam, cols, wd, U.seed_of(cols)), fam, stats, where)
            assert np.array_equal(bufs["a"], bufs["x"]), ("a != x in the wide family", where)
            if fam == families[0]:
                extra = dict(dtype=plan_dtype) if plan_dtype is not None else {}      # (option q3h_native: Wo, W1 / W3 and W2; QKV keeps the tiled form)
                _assert_plan(wk, "qkv", where, kind=kind, nj=nj, nchunk=int(kind == "classic"), npass=1, cols=cols, total_rows=3 * 32 * heads, norm=1, epi=U.EPI_PLAIN, dtype=wd)
                _assert_plan(wk, "ffn13", where, kind=kind, nj=nj, nchunk=int(kind == "classic"), npass=1, cols=cols, total_rows=256, norm=1, epi=U.EPI_GLU, **extra)
        _same_weights(wk, raw, cols)
        wk.close()


@pytest.mark.parametrize("wd,native", WIDE, ids=[ID[d] + ("-native" if n else "") for d, n in WIDE])
def test_columns_of_the_normalised_and_gated_inputs(wd, native):
    """QKV (PLAIN, norm 1) and W1 / W3 (GLU, norm 1) at every nj their inputs allow -- 1 .. 4 blocks per lane (B64 formats: 1 .. 2, dim
    <= 8192) --: one block into the last round, one block short of a full round, a full round, a ragged width, the smallest width"""
    stats = Stats("wide %s%s" % (ID[wd], " native" if native else ""))
    _wide_walk(wd, native, U.wide_edges(wd), stats, plan_dtype=U.Q3H_NATIVE if native else None)
    stats.report()


# ----------------------------------------------------------------------------- columns of the plain inputs
def _parts(wd):
    e = U.long_edges(wd)
    classic = [x for x in e if x[1] == "classic"]
    half = len(classic) // 2
    return {"low": classic[:half], "high": classic[half:], "long": [x for x in e if x[1] == "long"]}


LONG = [(d, n, p) for d, n in WIDE for p in ("low", "high", "long")]


def _long_walk(wd, native, edges, stats, plan_dtype=None):
    cap = dt.block_capacity(wd)
    for cols, kind, nj, nchunk in edges:
        lo, _ = U.last_round_cols(wd, cols)
        for fam in ("dense", "tail"):
            zero = {W.T_WV: lo, W.T_W1: lo, W.T_W3: lo} if fam == "tail" else None
            wk, cfg = _build(wd, 256, cols // 32, cols, native=native, zero_before=zero)
            raw = _weights(wk)
            model = _model(wk, cfg, raw)
            where = "%d columns %s" % (cols, fam)
            bufs, _ = _step(wk, cfg, model, U.make_input("dense", 256, wd, U.SEED_LONG), "dense", stats, where)
            if fam == "tail":
                for name in ("att", "t1"):
                    v = bufs[name].view(np.float16)
                    assert not v[:lo].any() and v[lo:].any(), ("the tail-only input of the plain launches is not tail-only", where, name)
            extra = dict(dtype=plan_dtype) if plan_dtype is not None else {}
            int8 = U.is_ax8(wd)
            # Wo reads the attention's quantised image while its row fits a lane's registers; past that (and on fp16 activations) it quantises itself
            _assert_plan(wk, "wo", where, kind=kind, nj=nj, nchunk=nchunk, cols=cols, total_rows=256, epi=U.EPI_RESIDUAL, norm=2 if (kind == "classic" and int8) else 0, **extra)
            _assert_plan(wk, "w2", where, kind=kind, nj=nj, nchunk=nchunk, cols=cols, total_rows=256, epi=U.EPI_RESIDUAL, norm=0, **extra)
            _assert_plan(wk, "ffn13", where, total_rows=cols, cols=256, epi=U.EPI_GLU, norm=1, **extra)
            _same_weights(wk, raw, where)
            wk.close()


@pytest.mark.parametrize("wd,native,part", LONG, ids=["%s%s-%s" % (ID[d], "-native" if n else "", p) for d, n, p in LONG])
def test_columns_of_the_plain_inputs(wd, native, part):
    """Wo (RESIDUAL, norm 2: the attention's quantised image; norm 0 on the long kernel) and W2 (RESIDUAL, norm 0) at every nj up to MAXNJ
    and on the chunked long-row kernel: its first width, a ragged one, the 2 -> 3 chunk change (Q8_B32T2) and 32768 columns; dense and
    tail-only activations.  W1 / W3 of these models have up to 32768 row pairs: several passes, the last one partial"""
    stats = Stats("long %s%s %s" % (ID[wd], " native" if native else "", part))
    _long_walk(wd, native, _parts(wd)[part], stats, plan_dtype=U.Q3H_NATIVE if native else None)
    stats.report()


# ----------------------------------------------------------------------------- the fp16-activation kernel
@pytest.mark.parametrize("wd", U.F16X_FORMATS, ids=[ID[d] for d in U.F16X_FORMATS])
def test_fp16_activation_kernel(wd):
    """k_dec_gemv_h (F16 weights and the block formats outside the int8 path): widths around one round of the lanes and at 8192 on the
    normalised inputs, 8224 / 16384 / 32768 on Wo and W2"""
    stats = Stats("f16x %s" % ID[wd])
    L = U.lane_round(wd)
    _wide_walk(wd, False, [(c, -(-c // L)) for c in U.f16x_wide_edges(wd)], stats, kind="f16x")
    _long_walk(wd, False, [(c, "f16x", -(-c // L), 0) for c in U.f16x_long_edges(wd)], stats)
    stats.report()


# ----------------------------------------------------------------------------- rows against the waves of the grid
ROW_FORMATS = (dt.Q4_B32T1A, dt.Q3H_B64T1, dt.Q8_B32T2)


@pytest.mark.parametrize("nj", (1, 2))
@pytest.mark.parametrize("wd", ROW_FORMATS, ids=[ID[d] for d in ROW_FORMATS])
def test_rows_against_the_waves_of_the_grid(wd, nj):
    """the W1 / W3 launch (row pairs (pass x RW + i) x W + wave, clamped first rows, the `full` fast path) with, from the plan on THIS
    device: the fewest row pairs a model can have (32, 64 for a B64 format: a grid of 2 - 8 workgroups), more than the W waves of the full grid but no more than
    RW x W (a partial first pass), and the smallest legal count past RW x W (a second pass of 32 rows; 64 for a B64 format).  Sign inputs: every launch is
    exactly comparable, so one wrong row shows."""
    stats = Stats("rows %s nj %d" % (ID[wd], nj))
    cols = nj * 64 * dt.block_capacity(wd)
    least = max(32, dt.block_capacity(wd))                 # (W2's columns: whole blocks)
    probe, _ = _build(wd, cols, 4, least, attn_out_scale=1e-12)
    p = probe.gemv_plan(0, "ffn13")
    probe.close()
    w_full = p["num_cus"] * p["threads"] // 64
    for rows, npass, partial in ((least, 1, 1), (w_full + least, 1, 1), (p["rw"] * w_full + least, 2, 1)):
        assert W.gemv_plan(wd, U.EPI_GLU, 1, cols, rows, p["num_cus"])["npass"] == npass
        wk, cfg = _build(wd, cols, 4, rows, attn_out_scale=1e-12)
        raw = _weights(wk)
        model = _model(wk, cfg, raw)
        where = "%d row pairs" % rows
        _step(wk, cfg, model, U.make_input("sign", cols, wd, U.seed_of(cols)), "sign", stats, where)
        _assert_plan(wk, "ffn13", where, kind="classic", nj=nj, npass=npass, partial=partial, total_rows=rows, rw=p["rw"], threads=p["threads"],
                     grid=min(p["num_cus"], -(-rows // (p["threads"] // 64))))
        _same_weights(wk, raw, where)
        wk.close()
    stats.report()


# ----------------------------------------------------------------------------- wirings
WIRINGS = {
    "act": (dict(is_glu=0), False, dict(ffn13=dict(epi=U.EPI_ACT, norm=1))),
    "stdnorm": (dict(norm_kind=1, is_glu=0, act_kind=1), False, dict(qkv=dict(epi=U.EPI_PLAIN, norm=0), ffn13=dict(epi=U.EPI_ACT, norm=0))),
    "parallel": (dict(parallel_attn=1), False, dict(wo=dict(epi=U.EPI_PLAIN, norm=2), ffn13=dict(epi=U.EPI_GLU, norm=0))),
    "bias": (dict(), True, {}),
    "scales": (dict(attn_out_scale=0.25, ffn_out_scale=0.5), False, {}),
}
WIRE = [(d, w) for d in (dt.Q4_B32T1A, dt.Q3H_B64T1) for w in WIRINGS]


@pytest.mark.parametrize("wd,wiring", WIRE, ids=["%s-%s" % (ID[d], w) for d, w in WIRE])
def test_wirings(wd, wiring):
    """the other epilogue / prologue instances at the nj 1 and 2 edges (a wide model with a == x and a long model per width): a plain (not gated) FFN (ACT, 1); the
    op-level std norm in front of (PLAIN, 0) and (ACT, 0); parallel attention -- Wo without the residual (PLAIN, 2), W1 / W3 on the stored
    normalised input (GLU, 0: after a step the buffer "hidden" holds the final norm's output, so the stored vector is checked through this
    launch, whose only input it is -- exactly on the sign family) --; biases on every matrix; attn_out_scale / ffn_out_scale"""
    cfg_over, bias, plans = WIRINGS[wiring]
    stats = Stats("wiring %s %s" % (ID[wd], wiring))
    for nj in (1, 2):
        for cols in U.nj_edges(wd, nj):
            # QKV and W1 / W3 at c columns on the wide shape (a == x, as in the wide family: W1 / W3 exact on sign), Wo and W2 on the long one
            for shape, roles in ((dict(dim=cols, heads=4, ffn=256), ("qkv", "ffn13")), (dict(dim=256, heads=cols // 32, ffn=cols), ("wo", "w2"))):
                wide = shape["heads"] == 4
                over = dict(cfg_over, attn_out_scale=1e-12) if wide else cfg_over
                wk, cfg = _build(wd, shape["dim"], shape["heads"], shape["ffn"], bias=bias, **over)
                raw = _weights(wk)
                model = _model(wk, cfg, raw)
                for fam in ("dense", "sign", "tail"):
                    where = "%d columns %s" % (cols, fam)
                    seed = U.seed_of(cols) if wide else U.SEED_LONG
                    _step(wk, cfg, model, U.make_input(fam, shape["dim"], wd, seed), fam, stats, where, roles=roles)
                for role in roles:
                    _assert_plan(wk, role, cols, kind="classic", nj=nj, nchunk=1, cols=cols, **plans.get(role, {}))
                _same_weights(wk, raw, cols)
                wk.close()
    stats.report()
