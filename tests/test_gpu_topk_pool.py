"""-m gpu: ifa_topk_pool (csrc/ifa_topk_pool.hip) against the NumPy restatement of SortedTopK's order (tests/pool_util.py).
The result is defined by a total order, so ids, value bits and counts are compared for equality, element for element."""
import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import worker as W
from oracle import sampling as S
from tests import gpu_util as g
from tests.pool_util import excluded_bits, pool_ref

pytestmark = pytest.mark.gpu

NS = [50, 1000, 32000, 32001, 151936]
KS = [1, 8, 50, 256]


def run_pool(rows_f16, k, excluded=None):
    rows_f16 = np.atleast_2d(rows_f16)
    bits = g.dev(excluded_bits(rows_f16.shape[1], excluded).view(np.int32)) if excluded is not None else None
    ids, vals, cnt = W.topk_pool(g.dev(rows_f16), k, bits, stream=torch.cuda.current_stream().cuda_stream)
    g.sync()
    return g.host(ids), g.host(vals).view(np.uint16), g.host(cnt)


def check(rows_f16, k, excluded=None, what=""):
    rows_f16 = np.atleast_2d(rows_f16)
    ids, vals, cnt = run_pool(rows_f16, k, excluded)
    for r in range(rows_f16.shape[0]):
        want_ids, want_bits = pool_ref(rows_f16[r], k, excluded if excluded is not None else ())
        c = int(cnt[r])
        assert c == want_ids.size, (what, r, k, c, want_ids.size)
        assert np.array_equal(ids[r, :c], want_ids), (what, r, k)
        assert np.array_equal(vals[r, :c], want_bits), (what, r, k)


def test_restatement_equals_the_oracle_on_a_tie_free_row():
    row = np.unique(np.random.default_rng(3).normal(0, 3.0, 8000).astype(np.float16))[:1000].copy()
    np.random.default_rng(4).shuffle(row)
    ids, bits = pool_ref(row, 50)
    want = S.sorted_top_k(row, 50)
    assert [int(i) for i in ids] == [i for i, _ in want] and [float(v) for v in bits.view(np.float16)] == [v for _, v in want]
    got_ids, got_bits, got_cnt = run_pool(row, 50)
    assert int(got_cnt[0]) == 50 and [int(i) for i in got_ids[0]] == [i for i, _ in want]


@pytest.mark.parametrize("rows", [1, 3, 32])
@pytest.mark.parametrize("n", NS)
def test_random_rows(n, rows):
    x = np.random.default_rng(n + rows).normal(0, 2.5, (rows, n)).astype(np.float16)      # (F16 normals: plenty of exact ties)
    for k in KS:
        check(x, k, what="normal")


def trouble_rows(n, k_edge):
    """rows built for trouble; k_edge: the pool length whose boundary the tie rows straddle"""
    rng = np.random.default_rng(n)
    u16 = lambda a: a.view(np.uint16)
    out = {}
    out["all_equal"] = np.full(n, np.float16(1.5))
    a = rng.normal(0, 1.0, n).astype(np.float16)
    a[rng.choice(n, min(300, n), replace=False)] = np.float16(9.0)       # 300 copies of the maximum: ties by id across every k
    out["max_copies"] = a
    z = -np.abs(rng.normal(0, 1.0, n)).astype(np.float16) - np.float16(0.5)      # all negative, then zeros of both signs on top
    zi = rng.choice(n, min(n, max(4, 2 * k_edge)), replace=False)
    z[zi] = np.float16(0.0)
    u16(z)[zi[::2]] = 0x8000                                              # -0.0 mixed with +0.0 at the boundary
    z[zi[: max(1, k_edge // 2)]] = np.float16(2.0)
    out["zeros"] = z
    i = rng.normal(0, 1.0, n).astype(np.float16)
    i[rng.choice(n, min(n, 7), replace=False)] = np.float16("inf")
    i[rng.choice(n, min(n, 7), replace=False)] = np.float16("-inf")
    out["infs"] = i
    s = np.zeros(n, np.float16)
    u16(s)[:] = rng.integers(0, 0x0400, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 15)      # subnormals (and zeros) of both signs
    out["subnormals"] = s
    q = rng.normal(0, 1.0, n).astype(np.float16)
    qi = rng.choice(n, n // 3, replace=False)
    u16(q)[qi[::2]] = 0x7E00
    u16(q)[qi[1::2]] = 0xFC01 + rng.integers(0, 0x3FE, qi[1::2].size).astype(np.uint16)       # negative NaNs with payloads
    out["nans"] = q
    out["all_nan"] = np.full(n, np.float16("nan"))
    neg = -np.abs(rng.normal(3, 1.0, n)).astype(np.float16)               # -inf among ordinary negatives, fewer finite than k
    neg[rng.choice(n, n // 2, replace=False)] = np.float16("-inf")
    out["neg_infs"] = neg
    return out


@pytest.mark.parametrize("n", NS)
def test_rows_built_for_trouble(n):
    for k in KS:
        t = trouble_rows(n, k)
        names = sorted(t)
        x = np.stack([t[m] for m in names])
        ids, vals, cnt = run_pool(x, k)
        for r, name in enumerate(names):
            want_ids, want_bits = pool_ref(x[r], k)
            c = int(cnt[r])
            assert c == want_ids.size, (name, n, k, c, want_ids.size)
            assert np.array_equal(ids[r, :c], want_ids), (name, n, k)
            assert np.array_equal(vals[r, :c], want_bits), (name, n, k)
        assert int(cnt[names.index("all_nan")]) == 0


@pytest.mark.parametrize("n", NS)
def test_excluded_ids(n):
    rng = np.random.default_rng(n + 7)
    x = rng.normal(0, 2.0, (3, n)).astype(np.float16)
    # all but 10 ids excluded: a short pool (count 10 < k) -- unless k is shorter still
    keep = rng.choice(n, 10, replace=False)
    most = np.setdiff1d(np.arange(n), keep)
    # the ids that would otherwise lead every row
    tops = np.unique(np.concatenate([pool_ref(x[r], 40)[0] for r in range(3)]))
    for k in KS:
        check(x, k, excluded=most, what="all but ten")
        ids, vals, cnt = run_pool(x, k, most)
        assert all(int(c) == min(k, 10) for c in cnt)
        check(x, k, excluded=tops, what="tops")
        ids, vals, cnt = run_pool(x, k, tops)
        assert not any(np.isin(ids[r, :int(cnt[r])], tops).any() for r in range(3))      # (slots past the count are unspecified)
        check(x, k, excluded=np.arange(n), what="everything")          # nothing left: count 0


def test_argument_checks():
    x = g.dev(np.zeros((1, 64), np.float16))
    ids = torch.zeros(512, dtype=torch.int32, device="cuda"); vals = torch.zeros(512, dtype=torch.int16, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = g.capi()
    assert L.ifa_topk_pool(g.p(x), 1, 64, 0, None, g.p(ids), g.p(vals), g.p(cnt), g.stream()) == -1        # IFA_ERR_ARG
    assert L.ifa_topk_pool(g.p(x), 1, 64, 257, None, g.p(ids), g.p(vals), g.p(cnt), g.stream()) == -1
    assert L.ifa_topk_pool(None, 1, 64, 8, None, g.p(ids), g.p(vals), g.p(cnt), g.stream()) == -1
    ia.check(L.ifa_topk_pool(g.p(x), 1, 64, 256, None, g.p(ids), g.p(vals), g.p(cnt), g.stream()))
    g.sync()
    assert int(cnt.item()) == 64 and g.host(ids)[:64].tolist() == list(range(64))                          # all equal: id order
