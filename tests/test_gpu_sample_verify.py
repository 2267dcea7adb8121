"""-m gpu: the verify kernel (csrc/ifa_sample_verify.hip, ifa_sample_verify_rows) against the same chain on the CPU
(ifa_sample_verify_host, itself pinned to a Python chain of ifa_sample_pool_host by tests/test_sample_verify_cpu.py), bit for bit:
tokens, indices, n_out, generator state and error word, over every acceptance outcome, the pool lengths at which the kernel
changes its path (64 / 65: one register per array or four), strides above the count, pools with runs of equal values and the four
sampled strategies plus greedy."""
import numpy as np
import pytest

from inferflow_amd import worker as W
from tests import sample_pools as P
from tests import verify_cases as V

pytestmark = pytest.mark.gpu

LENGTHS = [1, 50, 64, 65, 256]


def _launch(counts, ids, vals, params, draft, state0, err0=0, want_index=True):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = dev(np.array([state0], np.int64))
    err = dev(np.array([err0], np.int32))
    d = dev(np.asarray(draft, np.int32)) if len(draft) else None
    toks, idx, n_out = W.sample_verify_rows(dev(counts), dev(ids), dev(vals.view(np.int16)), dev(params.view(np.uint8).copy()), d, rng, err, want_index)
    torch.cuda.synchronize()
    return (toks.cpu().numpy(), idx.cpu().numpy() if idx is not None else None, int(n_out.item()), int(rng.item()), int(err.item()))


def _same(got, want):
    return np.array_equal(got[0], want[0]) and (got[1] is None or np.array_equal(got[1], want[1])) and got[2:] == want[2:]


def _case(pools, combo, seed, mismatch, k_stride):
    params = W.sample_params_array([combo])
    state0 = P.java_random_state(seed)
    draft = V.drafts_for(pools, params[0], state0, mismatch)
    counts, ids, vals = V.arrays(pools, k_stride)
    return counts, ids, vals, params, draft, state0


@pytest.mark.parametrize("n", LENGTHS)
def test_outcome_matrix_at_every_pool_length(n):
    bad, cases = [], 0
    for rows in (1, 2, 5, 8):
        for si, combo in enumerate(V.STRATEGIES):
            for mismatch in V.mismatch_rows(rows):
                pools = V.pools_of_length(n, rows, salt=10 * si + rows)
                # the stride equal to the count, and larger (junk behind the count must not be read)
                k_stride = n if (si + rows) % 2 == 0 else min(256, n + 7)
                c = _case(pools, combo, 50 + 13 * si + rows, mismatch, k_stride)
                got, want = _launch(*c), W.sample_verify_host(*c)
                cases += 1
                e = rows if mismatch is None else mismatch + 1
                if not _same(got, want) or want[2] != e or want[4] != 0:
                    bad.append((rows, combo, mismatch, got, want))
    assert not bad, "%d of %d cases differ from ifa_sample_verify_host, first: %r" % (len(bad), cases, bad[:3])


def test_pools_with_runs_of_equal_values():
    bad = []
    for rows in (2, 5, 8):
        for si, combo in enumerate(V.STRATEGIES[:4]):
            for mismatch in V.mismatch_rows(rows):
                pools = V.tie_pools(rows, salt=si + rows)
                assert all(P.has_ties(b) for _, b in pools)
                c = _case(pools, combo, 900 + si, mismatch, 256)
                got, want = _launch(*c), W.sample_verify_host(*c)
                if not _same(got, want):
                    bad.append((rows, combo, mismatch, got, want))
    assert not bad, "%d cases differ, first: %r" % (len(bad), bad[:3])


def test_mixed_lengths_in_one_launch_and_no_index_output():
    # rows of 1 / 50 / 64 / 65 / 256 entries side by side: each wave takes its own path
    pools = [V.pools_of_length(n, 1, salt=n)[0] for n in (65, 1, 256, 50, 64, 65, 2, 256)]
    for combo in V.STRATEGIES:
        for mismatch in V.mismatch_rows(8):
            c = _case(pools, combo, 4242, mismatch, 256)
            want = W.sample_verify_host(*c)
            assert _same(_launch(*c), want), (combo, mismatch)
            assert _same(_launch(*c, want_index=False), want), (combo, mismatch)


@pytest.mark.parametrize("combo", [V.STRATEGIES[2], V.STRATEGIES[4]])
def test_errors_only_at_a_reached_row_and_a_preset_error_word_is_left_alone(combo):
    rows, empty = 5, 3
    pools = V.pools_of_length(50, rows, salt=5)
    params = W.sample_params_array([combo])
    state0 = P.java_random_state(31)
    draft = V.drafts_for(pools, params[0], state0, None)
    pools[empty] = (np.zeros(0, np.int32), np.zeros(0, np.uint16))
    counts, ids, vals = V.arrays(pools, 50)
    got, want = _launch(counts, ids, vals, params, draft, state0), W.sample_verify_host(counts, ids, vals, params, draft, state0)
    assert _same(got, want) and got[2] == empty and got[4] == empty + 1
    got = _launch(counts, ids, vals, params, draft, state0, err0=42)
    assert got[4] == 42 and got[2] == empty
    # the same empty pool behind the first mismatch: no error, the generator moves by the emitted tokens only
    draft2 = draft.copy()
    draft2[1] += 1
    got, want = _launch(counts, ids, vals, params, draft2, state0), W.sample_verify_host(counts, ids, vals, params, draft2, state0)
    assert _same(got, want) and (got[2], got[4]) == (2, 0)
    assert got[3] == (state0 if combo[0] == P.GREEDY else V.advance(state0, 4))
    # a NaN value in a reached row cannot be drawn either (greedy never reads the values)
    pools[empty] = V.pools_of_length(50, 1, salt=6)[0]
    counts, ids, vals = V.arrays(pools, 50)
    vals[empty, 20] = 0x7E00
    got, want = _launch(counts, ids, vals, params, draft, state0), W.sample_verify_host(counts, ids, vals, params, draft, state0)
    assert _same(got, want)
    if combo[0] != P.GREEDY:
        assert got[2] == empty and got[4] == empty + 1


def test_an_unknown_strategy_fails_row_0():
    pools = V.pools_of_length(50, 3, salt=1)
    counts, ids, vals = V.arrays(pools, 50)
    params = W.sample_params_array([(5, 1.0, 0.9, 8, 0.05)])
    got = _launch(counts, ids, vals, params, [1, 2], 12345)
    assert got[2:] == (0, 12345, 1) and np.all(got[0] == -1) and np.all(got[1] == -1)


def test_two_launches_give_identical_bytes():
    pools = V.tie_pools(8, salt=2)
    c = _case(pools, V.STRATEGIES[0], 77, None, 256)
    a, b = _launch(*c), _launch(*c)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
