"""-m gpu: the worker's scoring prompt (ifa_model_forward_score) and the pool steps with option pool_lse against the float64
log-sum-exp of the SAME worker's logits (forward(..., logits_out) for the prompts -- identical rows by construction -- and the
"logits" tap for the steps), to the kernel's bound (tests/logprob_util.py); target logits bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth
from inferflow_amd.engine import InferenceEngine
from tests import engine_fixtures as fx
from tests.logprob_util import check_lse, lse_f64

pytestmark = pytest.mark.gpu

LENGTHS = [1, 5, 32, 40, 64, 200]


def _score_against_forward(wk, V, toks, prefix, what, row_by_row=False):
    n = len(toks)
    targets = np.append(toks[1:], -1).astype(np.int32)
    if n > 2:
        targets[1] = 0
        targets[2] = V - 1
    lg = torch.zeros((n, V), dtype=torch.float16, device="cuda")
    want_next = wk.forward(toks, prefix, lg)                    # (re-running a prompt at the same prefix rewrites the same cache rows)
    rows = lg.cpu().numpy()
    nxt, lse, tl = wk.forward_score(toks, prefix, targets)
    assert nxt == want_next == wk.forward(toks, prefix), what
    nxt2, lse2, tl2 = wk.forward_score(toks, prefix, targets)
    assert nxt2 == nxt and np.array_equal(lse.view(np.uint32), lse2.view(np.uint32)) and np.array_equal(tl.view(np.uint32), tl2.view(np.uint32)), what
    if row_by_row:               # (exact_order steps the rows one by one through ONE row of the worker's buffer: the last row is what remains)
        scored = wk.read_buffer("logits", nbytes=V * 2).view(np.uint16)
        assert np.array_equal(scored, rows[-1].view(np.uint16)), (what, "the scoring prompt's last row differs from forward(..., logits_out)")
    else:
        scored = wk.read_buffer("logits", nbytes=n * V * 2).view(np.uint16).reshape(n, V)
        assert np.array_equal(scored, rows.view(np.uint16)), (what, "the scoring prompt's rows differ from forward(..., logits_out)")
    worst = 0.0
    for i in range(n):
        worst = max(worst, check_lse(float(lse[i]), lse_f64(rows[i]), V, (what, i)))
        if targets[i] < 0:
            assert np.isnan(tl[i]), (what, i)
        else:
            assert tl[i].view(np.uint32) == np.float32(rows[i, targets[i]]).view(np.uint32), (what, i)
    print("%s: worst |err| / bound = %.3f" % (what, worst))


@pytest.mark.parametrize("shape", ["test_gqa", "test_mha"])
def test_forward_score_equals_the_logits_of_forward(shape):
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, dt.F16, max_ctx=320, quant_threshold=0, std=0.06)      # (test_mha: vocab 777, odd row starts)
    V = s["vocab"]
    rng = np.random.default_rng(7)
    for n in LENGTHS:
        toks = rng.integers(3, V, n).astype(np.int32)
        wk.reset()
        _score_against_forward(wk, V, toks, 0, (shape, n, "prefix 0"))
        head = rng.integers(3, V, 9).astype(np.int32)
        wk.reset()
        wk.forward(head, 0)
        _score_against_forward(wk, V, toks, len(head), (shape, n, "prefix 9"))
    for opt in ("exact_order", "perf_stat"):
        wk.set_option(opt, 1)
        for n in (1, 5, 40):
            toks = rng.integers(3, V, n).astype(np.int32)
            wk.reset()
            _score_against_forward(wk, V, toks, 0, (shape, n, opt), row_by_row=opt == "exact_order")
            wk.forward(toks[:3], 0)
            _score_against_forward(wk, V, toks, 3, (shape, n, opt, "prefix 3"), row_by_row=opt == "exact_order")
        wk.set_option(opt, 0)
    # bad arguments are codes
    L = ia.lib()
    z = np.zeros(4, np.int32); f = np.zeros(4, np.float32)
    zp, fp = z.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    bad = np.array([V, 0, 0, 0], np.int32)
    assert L.ifa_model_forward_score(wk._h, zp, 4, 0, bad.ctypes.data_as(C.c_void_p), fp, fp, None) == -1 and b"outside the vocabulary" in L.ifa_last_error()
    assert L.ifa_model_forward_score(wk._h, zp, 4, 0, None, fp, fp, None) == -1
    wk.close()


def test_pool_steps_with_the_lse_request():
    wk, _, s = synth.build("test_gqa", dt.Q4_B32T1A, dt.F16, max_ctx=64, quant_threshold=0, std=0.06)
    V = s["vocab"]
    prompt = np.random.default_rng(2).integers(3, V, 6).astype(np.int32)
    same = lambda a, b: a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    plain = wk.forward_pool(prompt, 0, 50)
    assert wk.pool_lse().size == 0                               # request off: nothing extra
    wk.reset()
    with_lse = wk.forward_pool_lse(prompt, 0, 50)
    assert same(plain, with_lse)
    row = wk.read_buffer("logits", nbytes=len(prompt) * V * 2).view(np.float16).reshape(len(prompt), V)[-1]
    check_lse(with_lse[3], lse_f64(row), V, "forward_pool")
    tok, pos = plain[0], len(prompt)
    for step in range(6):
        a = wk.decode_pool(tok, pos, 20)
        assert wk.pool_lse().size == 0
        b = wk.decode_pool_lse(tok, pos, 20)                     # (the same step again: same cache row rewritten, same logits)
        assert same(a, b)
        check_lse(b[3], lse_f64(wk.read_buffer("logits").view(np.float16)), V, ("decode_pool", step))
        assert wk.pool_lse().size == 1                           # still readable until the next pool step
        tok, pos = a[0], pos + 1
    for opt in ("fused", "exact_order"):                         # the other routes of the decode step
        wk.set_option(opt, 0 if opt == "fused" else 1)
        a = wk.decode_pool(tok, pos, 20)
        b = wk.decode_pool_lse(tok, pos, 20)
        assert same(a, b)
        check_lse(b[3], lse_f64(wk.read_buffer("logits").view(np.float16)), V, ("decode_pool", opt))
        wk.set_option(opt, 1 if opt == "fused" else 0)
    wk.close()
    # batched steps over three KV slots, ragged activity
    wk, _, s = synth.build("test_mha", dt.Q4_B32T1A, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)
    V = s["vocab"]
    wk.kv_slots(3)
    rng = np.random.default_rng(3)
    cur, pos = [int(t) for t in rng.integers(0, V, 3)], [0, 0, 0]
    for step in range(8):
        act = [0, 1, 2] if step % 3 else [2, 0]
        sel = list(range(len(act))) if step % 2 else [len(act) - 1]
        args = ([cur[q] for q in act], [pos[q] for q in act], act, 50, sel)
        nxt_a, pools_a = wk.decode_batch_pool(*args)
        assert wk.pool_lse().size == 0
        nxt_b, pools_b, lse = wk.decode_batch_pool_lse(*args)
        rows = wk.read_buffer("logits", nbytes=len(act) * V * 2).view(np.float16).reshape(len(act), V)
        assert np.array_equal(nxt_a, nxt_b) and lse.size == len(sel)
        for j, r in enumerate(sel):
            assert np.array_equal(pools_a[j][0], pools_b[j][0]) and np.array_equal(pools_a[j][1], pools_b[j][1])
            check_lse(float(lse[j]), lse_f64(rows[r]), V, ("decode_batch_pool", step, j))
        for j, q in enumerate(act):
            cur[q], pos[q] = int(nxt_a[j]), pos[q] + 1
    wk.close()


def test_a_partitioned_worker_refuses(tmp_path):
    ini, _ = fx.write_model_dir(str(tmp_path), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", maxq=4, devices="0&0")
    eng = InferenceEngine.from_ini(ini)
    L = ia.lib()
    h = L.ifa_engine_worker(eng._h, 0)
    assert h
    z = np.zeros(4, np.int32); f = np.zeros(4, np.float32)
    zp, fp = z.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    assert L.ifa_model_forward_score(C.c_void_p(h), zp, 4, 0, zp, fp, fp, None) == -4 and b"partitioned" in L.ifa_last_error()      # IFA_ERR_STATE
    # and the engine on top of it: no logprobs, no scoring
    assert eng.add_query([5, 6, 7], logprobs=0) < 0 and "multi-device" in eng._err()
    with pytest.raises(Exception, match="multi-device"):
        eng.score([5, 6, 7])
    assert eng.add_query([5, 6, 7]) > 0
    eng.close()
