"""-m gpu: every prompt attention kernel (csrc/ifa_attn.hip) against the oracle's arithmetic and against plain float64 math, at the
tile, block and switch-point edges of each, through the public entries ifa_attention and ifa_attention_rows on caller-owned tensors.

Kernels: k_attention (fewer than 4 queries, other head sizes, every row of ifa_attention_rows), k_attention_mfma with the score tile in
the LDS and -- past 2208 / 2304 / 2336 keys -- in the per-stream workspace, k_attention_2pass_ks (from 64 queries on: every real prompt)
and k_attention_2pass (through ifa_attention_two_pass_min_keys).  tests/prompt_attn_util.py has the matrix, the float64 reference, the
three input families (dense, flat, needle), the probed keys and the assertions; tests/test_prompt_attn_ref_cpu.py shows on the host
that a lost, doubled, mis-paired or leaked key, a lost block, an unscaled merge, unpermuted V columns, a clamped row, the wrong kv group
or ALiBi slope each move the float64 row by >= 5 x its bound and that check_rows rejects the oracle's output carrying them.

Every case asserts: ifa_attention_plan (with the settings read back from the library) names the kernel the case is meant for; both
bounds on every query row (out against float64 within max(2 x d_ref, one F16 ulp at max|out|), against oracle.attention within
6e-3 x max(1, max|V|)); the sentinel rows before and after `out` untouched; q, K and V unchanged; a second launch bit-identical.
Kernels that take the same input share its references, and stay within 4e-3 (x max(1, max|V|) on the flat and needle families) of each
other.  The measured figures are in docs/prompt_attention_edges.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from tests import gpu_util as g
from tests import prompt_attn_util as U

pytestmark = pytest.mark.gpu
PAD = 3                     # sentinel rows on either side of out
SENTINEL = 0x7B7B           # (F16 61280: no attention output of these inputs)
STATS = {}                  # kernel kind -> [err of every row of every case]
DEVICE_ERROR = []           # the first launch or copy that failed on the device: nothing more is started after it


class _Settings:
    """the two process-wide switches of ifa_attention set to `want`, put back on the way out"""

    def __init__(self, want):
        self.want = want

    def __enter__(self):
        L = g.capi()
        self.prev = (L.ifa_attention_two_pass_min(self.want[0]), L.ifa_attention_two_pass_min_keys(self.want[1]))
        return (L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1))

    def __exit__(self, *exc):
        L = g.capi()
        L.ifa_attention_two_pass_min(self.prev[0])
        L.ifa_attention_two_pass_min_keys(self.prev[1])


def _dev(a):
    return g.dev(np.array(a))           # (the references' arrays are read-only: the device gets a copy)


class _Device:
    """device work of one launch: an error of the runtime (not an assertion) ends the whole run -- after a fault nothing more is launched"""

    def __enter__(self):
        if DEVICE_ERROR:
            pytest.exit("an earlier launch failed on the device (%s): nothing more is started" % DEVICE_ERROR[0], returncode=3)

    def __exit__(self, kind, exc, tb):
        if exc is not None and not isinstance(exc, AssertionError):
            DEVICE_ERROR.append(repr(exc)[:200])


def _out_buffer(rows, cols):
    buf = torch.full((rows + 2 * PAD, cols), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, C.c_void_p(buf.data_ptr() + PAD * cols * 2)


def _read(buf, rows, where):
    h = buf.cpu().numpy()
    assert (h[:PAD] == SENTINEL).all() and (h[PAD + rows:] == SENTINEL).all(), ("a sentinel row around out was written", where)
    return h[PAD:PAD + rows].view(np.float16)


def _launch(case, stream=None):
    """one call of ifa_attention on the case's inputs, twice: (out [qt][heads * hd], the device tensors)"""
    sh = case.sh
    outs = []
    with _Device():
        dq, dk, dv = _dev(case.q), _dev(case.k_rows), _dev(case.v_rows)
        for _ in range(2):
            buf, ptr = _out_buffer(sh.qt, sh.heads * sh.hd)
            g.sync()            # (the sentinels are in place before a launch on another stream writes between them)
            ia.check(g.capi().ifa_attention(g.p(dq), g.p(dk), g.p(dv), sh.kvd, sh.n_ctx, sh.qt, sh.prefix, sh.heads, sh.kv_heads, sh.hd, sh.kq_scale,
                                            sh.alibi, 0, sh.heads, ptr, stream if stream is not None else g.stream()))
            g.sync()
            outs.append(_read(buf, sh.qt, case.tag))
    assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)), ("a second launch differs", case.tag)
    assert np.array_equal(g.host(dq).view(np.uint16), case.q.view(np.uint16)), ("q changed", case.tag)
    assert np.array_equal(dk.cpu().numpy(), case.k_rows) and np.array_equal(dv.cpu().numpy(), case.v_rows), ("K or V changed", case.tag)
    return outs[0]


def _record(kind, errs, case):
    STATS.setdefault(kind, []).append((float(errs.max()), case.tag))


def _walk(sh):
    """every case of a shape through every kernel that takes it; all of them are measured before the test fails"""
    failed, n, local = [], 0, {}
    for case in U.make_cases(sh):
        outs = {}
        for settings, kind in sh.routes():
            with _Settings(settings) as now:
                got = sh.plan(now)
                assert got["error"] == 0 and got["kind"] == kind, ("the plan names another kernel than the case is meant for", case.tag, U.KIND_NAMES[kind], got, now)
                out = _launch(case)
            n += 1
            outs[kind] = out
            try:
                errs = U.check_rows(out, case)
            except AssertionError as e:
                failed.append("%s: %s" % (U.KIND_NAMES[kind], e))
                continue
            _record(kind, errs, case)
            local.setdefault(kind, []).append(float(errs.max()))
        first = outs[sh.kind].astype(np.float64)
        cross = 4e-3 * (1.0 if case.family == "dense" else max(1.0, case.vmax))
        for kind, out in outs.items():
            d = float(np.abs(out.astype(np.float64) - first).max())
            if d > cross:
                failed.append("%s against %s: %.3g > %.3g (%s)" % (U.KIND_NAMES[kind], U.KIND_NAMES[sh.kind], d, cross, case.tag))
    for kind, e in local.items():
        e.sort()
        print("prompt-attn-edges %-60s %-14s %4d cases  median %.3f  worst %.3f" % (sh.id, U.KIND_NAMES[kind], len(e), e[len(e) // 2], e[-1]))
    assert not failed, "%d of %d launches: %s" % (len(failed), n, " | ".join(failed[:12]))


@pytest.mark.parametrize("sh", U.TWO_PASS, ids=[s.id for s in U.TWO_PASS])
def test_two_pass(sh):
    """64 queries per workgroup, key blocks split by parity over wave pairs; from 128 queries the same inputs through the 128-query
    variant and the staged kernel (two_pass_min 0), below that through the staged kernel where the shape says so"""
    _walk(sh)


@pytest.mark.parametrize("sh", U.MFMA, ids=[s.id for s in U.MFMA])
def test_staged_lds_tile(sh):
    _walk(sh)


WS_SHAPES = U.workspace_shapes()


@pytest.mark.parametrize("sh", WS_SHAPES, ids=[s.id for s in WS_SHAPES])
def test_lds_workspace_switch(sh):
    """the plan's last context on the LDS tile and the first one on the workspace, per head size"""
    _walk(sh)


@pytest.mark.parametrize("sh", U.SCALAR_SHAPES, ids=[s.id for s in U.SCALAR_SHAPES])
def test_scalar(sh):
    _walk(sh)


def test_workspace_reuse_on_one_stream():
    """long context, a shorter one (a smaller row stride over the stale tiles of the first), the long one again (no regrowth), all on ONE
    stream: each bit-identical to the same launch on a fresh stream, whose workspace is new"""
    long_, short = U.Shape(U.MFMA_WS, 2, 1, 128, U.F16, 2400 - 40, 40), U.Shape(U.MFMA_WS, 2, 1, 128, U.F16, 2209 - 33, 33)
    assert long_.plan()["sg_nkp"] > short.plan()["sg_nkp"] > 0
    cases = {s.id: next(U.make_cases(s, ("dense",))) for s in (long_, short)}
    L = g.capi()
    shared = torch.cuda.Stream()
    streams = [shared]
    try:
        for step, sh in enumerate((long_, short, long_)):
            case = cases[sh.id]
            assert sh.plan((L.ifa_attention_two_pass_min(-1), L.ifa_attention_two_pass_min_keys(-1)))["kind"] == U.MFMA_WS
            fresh = torch.cuda.Stream()
            streams.append(fresh)
            torch.cuda.synchronize()
            a = _launch(case, C.c_void_p(shared.cuda_stream))
            b = _launch(case, C.c_void_p(fresh.cuda_stream))
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), ("reused workspace differs from a fresh one", step, sh.id)
            _record(U.MFMA_WS, U.check_rows(a, case), case)
    finally:
        torch.cuda.synchronize()
        for s in streams:
            ia.check(L.ifa_gemm_release_stream(C.c_void_p(s.cuda_stream)))          # (frees the stream's score workspace)


class _AttnRow(C.Structure):
    _fields_ = [("kc", C.c_void_p), ("vc", C.c_void_p), ("n_ctx", C.c_int), ("pad", C.c_int)]


@pytest.mark.parametrize("batch", U.ROWS_BATCHES, ids=["rows%d-h%dkv%d-hd%d-%s%s" % (len(b[0]), b[1], b[2], b[3], "f16" if b[4] == U.F16 else "q8", "-alibi" if b[5] else "") for b in U.ROWS_BATCHES])
def test_rows_entry(batch):
    """ifa_attention_rows: every row one query on its own cache tensors and context; the LDS is sized by the longest row; every row is
    checked as a one-query case against its own keys only"""
    ctxs, heads, kv_heads, hd, kvd, alibi = batch
    shapes = U.rows_batch_shapes(batch)
    per_row = [{f: list(U.make_cases(s, (f,))) for f in ("dense", "flat", "needle")} for s in shapes]
    n_rows, max_ctx = len(ctxs), max(ctxs)
    p = U.plan(kvd, max_ctx, n_rows, 0, heads, kv_heads, hd, rows_mode=1)
    assert (p["error"], p["kind"], p["grid"]) == (0, U.SCALAR, (heads, n_rows)) and p["lds"] == (max_ctx * 2 + 15) // 16 * 16 + 64
    rounds = [("dense", 0), ("flat", 0)] + [("needle", i) for i in range(max(len(r["needle"]) for r in per_row))]
    failed, local = [], []
    for family, i in rounds:
        cases = [(r[family][i % len(r[family])] if r[family] else r["dense"][0]) for r in per_row]        # (a one-key row has its dense case only)
        dq = _dev(np.concatenate([c.q for c in cases]))
        dk, dv = [_dev(c.k_rows) for c in cases], [_dev(c.v_rows) for c in cases]
        recs = (_AttnRow * n_rows)(*[_AttnRow(dk[r].data_ptr(), dv[r].data_ptr(), ctxs[r], 0) for r in range(n_rows)])
        drows = g.dev(np.frombuffer(bytes(recs), np.uint8).copy())
        outs = []
        with _Device():
            for _ in range(2):
                buf, ptr = _out_buffer(n_rows, heads * hd)
                ia.check(g.capi().ifa_attention_rows(g.p(dq), g.p(drows), kvd, n_rows, max_ctx, heads, kv_heads, hd, shapes[0].kq_scale, alibi, 0, heads, ptr, g.stream()))
                g.sync()
                outs.append(_read(buf, n_rows, (family, i)))
        assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)), ("a second launch differs", family, i)
        assert np.array_equal(drows.cpu().numpy(), np.frombuffer(bytes(recs), np.uint8)), "the row records changed"
        for r, c in enumerate(cases):
            assert np.array_equal(dk[r].cpu().numpy(), c.k_rows) and np.array_equal(dv[r].cpu().numpy(), c.v_rows), ("K or V changed", c.tag)
            try:
                errs = U.check_rows(outs[0][r:r + 1], c)
            except AssertionError as e:
                failed.append("row %d: %s" % (r, e))
                continue
            STATS.setdefault("rows", []).append((float(errs.max()), c.tag))
            local.append(float(errs.max()))
    local.sort()
    print("prompt-attn-edges rows %-40s %4d rows  median %.3f  worst %.3f" % (ctxs, len(local), local[len(local) // 2] if local else 0, local[-1] if local else 0))
    assert not failed, "%d rows: %s" % (len(failed), " | ".join(failed[:12]))


def test_summary():
    """(runs last in this file) the figures of docs/prompt_attention_edges.md: err = max|out - float64| / max(d_ref, ulp / 2) per kernel"""
    for kind in list(range(5)) + ["rows"]:
        s = sorted(STATS.get(kind, []))
        if s:
            print("prompt-attn-edges total %-14s %5d cases  median %.3f  worst %.3f (%s)" % (U.KIND_NAMES[kind] if kind != "rows" else "rows entry", len(s), s[len(s) // 2][0], s[-1][0], s[-1][1]))
    assert all(e <= 2.0 for v in STATS.values() for e, _ in v)
