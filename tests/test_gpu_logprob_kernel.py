"""-m gpu: ifa_logsumexp_rows (csrc/ifa_logprob.hip) against the float64 NumPy statement of the row log-sum-exp.
Required of every finite case: |lse_dev - lse_f64| <= (2 ceil(n / 2048) + 24) 2^-24 + 2^-23 max(1, |lse_f64|) (tests/logprob_util.py:
the worst-case fp32 bound of the kernel's prescribed structure), the target logit bit-exact, NaN out exactly for NaN / +inf /
all -inf rows, two runs bit-identical."""
import numpy as np
import pytest
import torch

from inferflow_amd import worker as W
from tests import gpu_util as g
from tests.logprob_util import bound, lse_f64

pytestmark = pytest.mark.gpu

NS = [8, 1000, 2047, 2048, 2049, 32000, 32001, 50257, 151936]
DISTS = [(1.0, 0.0), (4.0, 0.0), (8.0, -20.0), (0.01, 7.0), (30.0, 0.0)]      # (sigma, mu)


def lse_rows_f64(x):
    if x.shape[0] > 64:          # (in slices: the float64 temporaries of a 600 x 151936 block are gigabytes)
        return np.concatenate([lse_rows_f64(x[i:i + 64]) for i in range(0, x.shape[0], 64)])
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        out = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    bad = np.isnan(x).any(axis=1) | np.isposinf(x).any(axis=1) | np.isneginf(x).all(axis=1)
    out[bad] = np.nan
    return out


def run(x16, n=None, row_idx=None, targets=None, split=True):
    xd = g.dev(x16)
    ri = g.dev(np.asarray(row_idx, np.int32)) if row_idx is not None else None
    tg = g.dev(np.asarray(targets, np.int32)) if targets is not None else None
    lse, tl = W.logsumexp_rows(xd, n=n, row_idx=ri, targets=tg, split=split, stream=torch.cuda.current_stream().cuda_stream)
    g.sync()
    return g.host(lse), (g.host(tl) if tl is not None else None)


def check(x16, n=None, row_idx=None, targets=None, what="", split=True):
    """x16 [rows_avail][stride]; returns the largest |error| / bound"""
    n = x16.shape[1] if n is None else n
    rows = list(range(x16.shape[0])) if row_idx is None else list(row_idx)
    lse, tl = run(x16, n, row_idx, targets, split)
    lse2, tl2 = run(x16, n, row_idx, targets, split)
    assert np.array_equal(lse.view(np.uint32), lse2.view(np.uint32)), (what, "two runs differ")
    want = lse_rows_f64(x16[rows][:, :n])
    assert np.array_equal(np.isnan(lse), np.isnan(want)), (what, lse[:8], want[:8])
    ok = ~np.isnan(want)
    err = np.abs(lse[ok].astype(np.float64) - want[ok])
    bnd = np.array([bound(n, w) for w in want[ok]])
    worst = float((err / bnd).max()) if err.size else 0.0
    print("%s n=%d rows=%d: worst |err| / bound = %.3f" % (what, n, len(rows), worst))
    assert (err <= bnd).all(), (what, n, float(err.max()), float(bnd.min()), worst)
    if targets is not None:
        assert np.array_equal(tl.view(np.uint32), tl2.view(np.uint32))
        for j, (r, t) in enumerate(zip(rows, targets)):
            if t < 0:
                assert np.isnan(tl[j]), (what, j, t)
            else:
                assert tl[j].view(np.uint32) == np.float32(x16[r, t]).view(np.uint32), (what, j, t)
    return worst


def normal_rows(rows, n, sigma, mu, seed):
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        x = (rng.standard_normal((rows, n), dtype=np.float32) * np.float32(sigma) + np.float32(mu)).astype(np.float16)
    return np.clip(x, np.float16(-65504), np.float16(65504))     # (sigma 30 never reaches it; the clip states the intent)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_normal_rows_few(n, rows):
    for d, (sigma, mu) in enumerate(DISTS):
        x = normal_rows(rows, n, sigma, mu, 1000 * d + n + rows)
        tg = [0, n - 1, -1][:rows] if rows == 3 else [n - 1]
        check(x, targets=tg, what="N(%g,%g)" % (mu, sigma))


@pytest.mark.parametrize("n", NS)
def test_normal_rows_many(n):
    """600 rows (a prompt): one workgroup per row.  Every distribution up to 32001 ids, one per size above (the block is 180 MB)"""
    dists = DISTS if n <= 32001 else [DISTS[NS.index(n) % len(DISTS)]]
    for d, (sigma, mu) in enumerate(dists):
        x = normal_rows(600, n, sigma, mu, 77 * d + n)
        tg = np.random.default_rng(n + d).integers(-1, n, 600)
        tg[0], tg[1], tg[2] = 0, n - 1, -1
        check(x, targets=tg, what="600 x N(%g,%g)" % (mu, sigma))


@pytest.mark.parametrize("rows_sel", [[0], [4, 1, 3], list(range(5)) * 120])
@pytest.mark.parametrize("n", NS)
def test_row_index_and_a_stride_larger_than_n(n, rows_sel):
    """rows picked by index out of a [5][n + 13] block (odd strides: rows start at any 2-byte address), the 13 halfs past n are
    huge and must not be read into the result"""
    stride = n + 13
    x = normal_rows(5, stride, 4.0, 0.0, n + len(rows_sel))
    x[:, n:] = np.float16(60000.0)
    tg = [(0, n - 1, -1)[j % 3] for j in range(len(rows_sel))]
    check(x, n=n, row_idx=rows_sel, targets=tg, what="row_idx")
    check(x, n=n, what="stride")            # without an index: rows 0..4 at the same stride
    check(x, n=n, what="no workspace", split=False)


@pytest.mark.parametrize("n,rows", [(n, r) for n in (8, 2049, 32001, 151936) for r in (1, 3)] + [(8, 600), (2049, 600), (32001, 600)])
def test_hostile_rows(n, rows):
    rng = np.random.default_rng(n + rows)
    inf = np.float16("inf")
    base = normal_rows(rows, n, 2.0, 0.0, n)
    cases = {}
    x = base.copy(); x[:] = np.float16(3.25); cases["all equal"] = (x, False)
    x = base.copy(); x[:, rng.integers(0, n, max(n // 3, 1))] = -inf; cases["-inf entries"] = (x, False)
    x = base.copy(); x[:, : n - 1] = -inf; cases["one finite entry"] = (x, False)
    x = base.copy(); x[:, rng.integers(0, n, 5)] = np.float16(65504); x[:, rng.integers(0, n, 5)] = np.float16(-65504); cases["+-65504"] = (x, False)
    x = base.copy(); x[:] = np.float16(-65504); cases["all -65504"] = (x, False)
    x = base.copy(); x[:] = -inf; cases["only -inf"] = (x, True)
    x = base.copy(); x[:, n // 2] = np.float16("nan"); cases["a NaN"] = (x, True)
    x = base.copy(); x[:] = -inf; x[:, n - 1] = np.float16("nan"); cases["a NaN among -inf"] = (x, True)
    x = base.copy(); x[:, n - 1] = inf; cases["+inf"] = (x, True)
    x = base.copy(); x[:, 0] = inf; x[:, 1:] = -inf; cases["+inf among -inf"] = (x, True)
    for what, (x, nan_out) in cases.items():
        lse, _ = run(x)
        assert np.isnan(lse).all() == nan_out and np.isnan(lse).any() == nan_out, (what, lse[:4])
        check(x, targets=[(0, n - 1, -1)[j % 3] for j in range(rows)], what=what)
    # NaN stays in its row: a block where only row 1 is poisoned
    if rows >= 3:
        x = base.copy(); x[1, n - 1] = np.float16("nan")
        lse, _ = run(x)
        assert np.isnan(lse[1]) and not np.isnan(np.delete(lse, 1)).any()


def test_split_and_unsplit_rows_agree_within_the_bound():
    """the same row through one workgroup and through the split + combine: both inside the bound of the float64 value"""
    for n in (32000, 151936):
        x = normal_rows(1, n, 4.0, 0.0, n)
        a, _ = run(x, split=True)
        b, _ = run(x, split=False)
        want = lse_f64(x[0])
        assert abs(float(a[0]) - want) <= bound(n, want) and abs(float(b[0]) - want) <= bound(n, want)


def test_bad_arguments_are_codes():
    import ctypes as C
    import inferflow_amd as ia
    L = ia.lib()
    x = g.dev(np.zeros((1, 64), np.float16)); out = torch.zeros(1, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.ifa_logsumexp_rows(None, 64, None, 1, 64, None, p(out), None, None, None) == -1
    assert L.ifa_logsumexp_rows(p(x), 32, None, 1, 64, None, p(out), None, None, None) == -1          # stride below n
    assert L.ifa_logsumexp_rows(p(x), 64, None, 1, 64, None, p(out), p(out), None, None) == -1        # target output without targets
    assert L.ifa_logsumexp_rows(p(x), 64, None, 0, 64, None, p(out), None, None, None) == -1
