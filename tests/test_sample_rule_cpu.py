"""No GPU: the draw rule of the device sampler (csrc/ifa_sample_rule.h) compiled for the host, ifa_sample_pool_host, against the
host sampler that is pinned to the reference (ifa_sampling_choose_from_pool): same pool, same seed, consecutive draws -- the token
of every draw (so the generator position), the cut length, the pool's ids and probabilities bit for bit; the sort's order against
oracle.sampling.std_sort on every tie pattern."""
import numpy as np
import pytest

from inferflow_amd import engine as E
from inferflow_amd import worker as W
from inferflow_amd._capi import IfaError
from oracle import sampling as S
from tests import sample_pools as P

DRAWS = 3
TIES, PLAIN, INFS, NATURAL = P.tie_pools(), P.plain_pools(), P.inf_pools(), P.natural_pools()
COMBOS = P.combos()


def _bits32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _compare(pool, combo, seed):
    name, ids, bits = pool
    strategy, temperature, top_p, max_k, min_p = combo
    want = E.sampling_choose_from_pool(ids, bits, strategy, temperature=temperature, seed=seed, n_draws=DRAWS, max_k=max_k, top_p=top_p,
                                       pool_size=len(ids), min_p=min_p)
    params = W.sample_params_array([combo])[0]
    state = P.java_random_state(seed)
    for d in range(DRAWS):
        tok, idx, cut, w, order, state = W.sample_pool_host(ids, bits, params, state)
        where = "%s %r seed %d draw %d" % (name, combo, seed, d)
        assert tok == want[0][d], where                              # the token: same sort, same cut, same generator position
        assert cut == len(want[2]), where
        assert [int(i) for i in order[:cut]] == want[2], where
        assert np.array_equal(_bits32(w[:cut]), _bits32(want[3])), where
        assert 0 <= idx < cut and int(order[idx]) == tok, where
    assert state == P.java_random_state(seed, DRAWS)                 # two generator steps per draw, nothing else


@pytest.mark.parametrize("group", ["ties", "plain", "inf"])
def test_host_rule_equals_the_host_sampler_on_every_parameter_combination(group):
    pools = {"ties": TIES, "plain": PLAIN, "inf": INFS}[group]
    for pi, pool in enumerate(pools):
        for ci, combo in enumerate(COMBOS):
            _compare(pool, combo, seed=1000 + 31 * pi + ci)


def test_host_rule_equals_the_host_sampler_on_natural_pools():
    tied = sum(P.has_ties(bits) for _, _, bits in NATURAL)
    assert 2 * tied >= len(NATURAL), "only %d of %d pools hold equal values: the case is not covered" % (tied, len(NATURAL))
    for pi, pool in enumerate(NATURAL):
        for j in range(4):
            _compare(pool, COMBOS[(7 * pi + 37 * j) % len(COMBOS)], seed=5000 + pi)


@pytest.mark.parametrize("pool", TIES + PLAIN + INFS, ids=lambda p: p[0])
def test_sorted_order_equals_std_sort(pool):
    name, ids, bits = pool
    vals = bits.view(np.float16).astype(np.float32)
    want = S.std_sort([(int(i), np.float32(v)) for i, v in zip(ids, vals)], lambda x, y: x[1] > y[1])
    params = W.sample_params_array([(P.TOP_K, 1.0, 1.0, 300, 0.0)])[0]
    _, _, _, _, order, _ = W.sample_pool_host(ids, bits, params, P.java_random_state(1))
    assert [int(i) for i in order] == [i for i, _ in want]


def test_natural_pools_sorted_order_equals_std_sort():
    params = W.sample_params_array([(P.TOP_K, 1.0, 1.0, 300, 0.0)])[0]
    for name, ids, bits in NATURAL:
        vals = bits.view(np.float16).astype(np.float32)
        want = S.std_sort([(int(i), np.float32(v)) for i, v in zip(ids, vals)], lambda x, y: x[1] > y[1])
        _, _, _, _, order, _ = W.sample_pool_host(ids, bits, params, P.java_random_state(1))
        assert [int(i) for i in order] == [i for i, _ in want], name


def test_an_all_inf_pool_does_what_the_host_sampler_does():
    for pool in INFS:
        if pool[0].startswith("all_inf"):
            for combo in COMBOS[::5]:
                _compare(pool, combo, seed=77)


def test_an_empty_pool_is_an_error_and_yields_no_token():
    params = W.sample_params_array([(P.TOP_P, 1.0, 0.9, 8, 0.05)])[0]
    with pytest.raises(IfaError) as e:
        W.sample_pool_host(np.zeros(0, np.int32), np.zeros(0, np.uint16), params, 5)
    assert e.value.code == -4 and "empty pool" in str(e.value)      # IFA_ERR_STATE


def test_greedy_takes_the_first_id_and_leaves_the_generator_alone():
    name, ids, bits = TIES[0]
    params = W.sample_params_array([(P.GREEDY, 1.0, 0.9, 8, 0.05)])[0]
    tok, idx, cut, _, _, state = W.sample_pool_host(ids, bits, params, 123456789)
    assert (tok, idx, cut, state) == (int(ids[0]), 0, 1, 123456789)


def test_bad_arguments_are_refused():
    name, ids, bits = PLAIN[3]
    with pytest.raises(IfaError) as e:
        W.sample_pool_host(ids, bits, W.sample_params_array([(10, 1.0, 0.9, 8, 0.05)])[0], 1)      # mirostat: not the device's
    assert e.value.code == -1
    nan = bits.copy()
    nan[2] = 0x7E00
    with pytest.raises(IfaError) as e:
        W.sample_pool_host(ids, nan, W.sample_params_array([(P.TOP_P, 1.0, 0.9, 8, 0.05)])[0], 1)
    assert e.value.code == -1 and "NaN" in str(e.value)


def test_lcg_known_answers():
    # java.util.Random, seed 42: nextDouble() = 0.7275636800328681.  256 equal weights at temperature 1 are 2^-8 each (exact), the
    # interval starts are i / 256 (exact), so the draw's index is floor(256 * nextDouble()) and the state is the published LCG's
    assert S.JavaRandom(42).next_double() == 0.7275636800328681
    name, ids, bits = P._from_values("eq", np.full(256, 1.0))
    params = W.sample_params_array([(P.TOP_K, 1.0, 1.0, 300, 0.0)])[0]
    tok, idx, cut, w, order, state = W.sample_pool_host(ids, bits, params, W.rng_state_of_seed(42))
    assert cut == 256 and np.all(w == np.float32(1.0 / 256))
    assert idx == int(256 * 0.7275636800328681) == 186 and tok == int(order[186])
    ref = S.JavaRandom(42)
    ref.next_double()
    assert state == ref.seed == P.java_random_state(42, 1)
    assert E.random_doubles(42, 1)[0] == 0.7275636800328681          # the host sampler's generator: the stream the device continues
