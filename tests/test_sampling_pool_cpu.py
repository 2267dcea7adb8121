"""The host half of device-side sampling pools, without a GPU: ifa_sampling_choose_from_pool fed the row's candidate pool
(SortedTopK: what ifa_topk_pool builds on the device) must do exactly what ifa_sampling_choose_ex does on the full row --
same selected ids over consecutive draws (so the same generator position), same token pool, same Mirostat / FSD state."""
import numpy as np
import pytest

from inferflow_amd import engine as E
from oracle import sampling as S
from tests.pool_util import pool_ref

V, POOL = 1000, 50
ALL = [S.STD, S.GREEDY, S.TOP_K, S.TOP_P, S.FSD, S.RANDOM_FSD, S.MIN_P, S.TFS, S.TYPICAL, S.MIROSTAT]


def _rows():
    rng = np.random.default_rng(17)
    normal = rng.normal(0, 2.0, V).astype(np.float16)
    ties = rng.normal(0, 2.0, V).astype(np.float16)
    top = np.sort(ties.astype(np.float32))[-45]
    ties[rng.choice(V, 30, replace=False)] = np.float16(top)        # equal values straddling entry 50 of the pool
    nans = rng.normal(0, 2.0, V).astype(np.float16)
    nans[rng.choice(V, 200, replace=False)] = np.float16("nan")
    nans.view(np.uint16)[5] = 0xFE01                                 # a negative NaN with a payload
    short = np.full(V, np.float16("nan"))
    short[rng.choice(V, 20, replace=False)] = rng.normal(0, 2.0, 20).astype(np.float16)      # fewer than pool_size entries
    return {"normal": normal, "ties": ties, "nans": nans, "short": short}


ROWS = _rows()


def test_restated_order_equals_the_oracles_on_a_tie_free_row():
    row = np.unique(np.random.default_rng(3).normal(0, 3.0, 4 * V).astype(np.float16))[:V].copy()
    np.random.default_rng(4).shuffle(row)
    ids, bits = pool_ref(row, POOL)
    want = S.sorted_top_k(row, POOL)
    assert [int(i) for i in ids] == [i for i, _ in want]
    assert [float(v) for v in bits.view(np.float16)] == [v for _, v in want]


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("strategy", ALL)
@pytest.mark.parametrize("temperature", [1.0, 0.7, 0.0005])
@pytest.mark.parametrize("seed", [1, 12345])
def test_choose_from_pool_equals_choose_on_the_row(name, strategy, temperature, seed):
    row = ROWS[name]
    text = [5, 9, 5, 9, 7, 5, 9]
    draws = 12 if strategy in (S.FSD, S.RANDOM_FSD) else 6           # consecutive draws share the generator (and the FSD n-gram model)
    k = 1 if strategy == S.GREEDY else min(POOL, V)
    cid, cbits = pool_ref(row, k)
    want = E.sampling_choose_ex(row, strategy, temperature=temperature, seed=seed, n_draws=draws, pool_size=POOL, text=text)
    got = E.sampling_choose_from_pool(cid, cbits, strategy, temperature=temperature, seed=seed, n_draws=draws, pool_size=POOL, text=text)
    assert got[0] == want[0]                                         # selected ids of every draw
    assert got[2] == want[2]                                         # token pool of the last draw
    assert np.array_equal(np.float32(got[1]).view(np.uint32), np.float32(want[1]).view(np.uint32))
    assert np.array_equal(np.float32(got[3]).view(np.uint32), np.float32(want[3]).view(np.uint32))
    assert np.float32(got[4]).view(np.uint32) == np.float32(want[4]).view(np.uint32)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_mirostat_mu_follows_over_consecutive_calls(name):
    row = ROWS[name]
    cid, cbits = pool_ref(row, POOL)
    mu_a = mu_b = None
    for call in range(5):
        a = E.sampling_choose_ex(row, S.MIROSTAT, seed=40 + call, n_draws=1, mu=mu_a, pool_size=POOL)
        b = E.sampling_choose_from_pool(cid, cbits, S.MIROSTAT, seed=40 + call, n_draws=1, mu=mu_b, pool_size=POOL)
        assert a[0] == b[0] and a[2] == b[2]
        mu_a, mu_b = a[4], b[4]
        assert np.float32(mu_a).view(np.uint32) == np.float32(mu_b).view(np.uint32) and mu_a == mu_a


def test_an_empty_pool_selects_nothing_like_an_all_nan_row():
    row = np.full(V, np.float16("nan"))
    want = E.sampling_choose_ex(row, S.TOP_P, seed=3, n_draws=1)
    got = E.sampling_choose_from_pool([], [], S.TOP_P, seed=3, n_draws=1)
    assert want[2] == got[2] == []
