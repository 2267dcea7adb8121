"""-m gpu: the draw kernel (csrc/ifa_sample_pool.hip, ifa_sample_pool_rows) against the same rule compiled for the host
(ifa_sample_pool_host, itself pinned to the host sampler by tests/test_sample_rule_cpu.py): the pools of tests/sample_pools.py as
rows of ONE launch with mixed strategies and seeds, then 64 more launches on the advancing generator states.  Tokens, indices,
probabilities and generator states are compared exactly."""
import numpy as np
import pytest

from inferflow_amd import worker as W
from tests import sample_pools as P

pytestmark = pytest.mark.gpu

K = 256
LAUNCHES = 65


def _rows():
    pools = P.tie_pools() + P.plain_pools() + P.inf_pools() + P.natural_pools()
    combos = P.combos()
    rows = []
    for i, (name, ids, bits) in enumerate(pools):
        combo = combos[(11 * i) % len(combos)]
        if i % 29 == 5:
            combo = (P.GREEDY, 1.0, 0.9, 8, 0.05)
        rows.append((name, ids, bits, combo, 900 + 7 * i))
    return rows


def _upload(rows):
    import torch
    n = len(rows)
    counts = np.zeros(n, np.int32)
    ids = np.zeros((n, K), np.int32)
    vals = np.zeros((n, K), np.uint16)
    states = np.zeros(n, np.int64)
    for r, (_, i, b, _, seed) in enumerate(rows):
        counts[r] = len(i)
        ids[r, :len(i)] = i
        vals[r, :len(i)] = b
        states[r] = P.java_random_state(seed)
    params = W.sample_params_array([c for _, _, _, c, _ in rows])
    dev = lambda a: torch.from_numpy(a).cuda()
    return (dev(counts), dev(ids), dev(vals.view(np.int16)), dev(params.view(np.uint8).copy()), dev(states)), params


def test_rows_of_one_launch_and_64_more_on_advancing_states():
    import torch
    rows = _rows()
    (counts, ids, vals, params_dev, states), params = _upload(rows)
    n = len(rows)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    weights = torch.zeros((n, K), dtype=torch.float32, device="cuda")
    toks, idxs = [], []
    for launch in range(LAUNCHES):
        t, i = W.sample_pool_rows(counts, ids, vals, params_dev, states, err, weights if launch == 0 else None)
        toks.append(t)
        idxs.append(i)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    toks = torch.stack(toks).cpu().numpy()
    idxs = torch.stack(idxs).cpu().numpy()
    weights = weights.cpu().numpy()
    states = states.cpu().numpy()
    bad = []
    for r, (name, pid, bits, combo, seed) in enumerate(rows):
        st = P.java_random_state(seed)
        for launch in range(LAUNCHES):
            tok, idx, cut, w, order, st = W.sample_pool_host(pid, bits, params[r], st)
            if (int(toks[launch, r]), int(idxs[launch, r])) != (tok, idx):
                bad.append((name, combo, launch, int(toks[launch, r]), tok, int(idxs[launch, r]), idx))
                break
            if launch == 0 and combo[0] != P.GREEDY:
                got = weights[r, :len(pid)].view(np.uint32)
                if not np.array_equal(got, w.view(np.uint32)):
                    j = int(np.nonzero(got != w.view(np.uint32))[0][0])
                    bad.append((name, combo, "weight", j, float(weights[r, j]), float(w[j])))
                    break
        else:
            if int(states[r]) != st:
                bad.append((name, combo, "state", int(states[r]), st))
    assert not bad, "%d of %d rows differ from ifa_sample_pool_host, first: %r" % (len(bad), n, bad[:5])


def test_an_empty_row_sets_the_error_word_and_leaves_the_others_intact():
    import torch
    rows = _rows()[:40]
    (counts, ids, vals, params_dev, states), params = _upload(rows)
    empty = 13
    counts[empty] = 0
    before = states.clone()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    toks, idxs = W.sample_pool_rows(counts, ids, vals, params_dev, states, err)
    torch.cuda.synchronize()
    assert int(err.item()) == empty + 1
    toks, idxs, states = toks.cpu().numpy(), idxs.cpu().numpy(), states.cpu().numpy()
    assert (int(toks[empty]), int(idxs[empty])) == (-1, -1) and int(states[empty]) == int(before[empty].item())
    for r, (name, pid, bits, combo, seed) in enumerate(rows):
        if r == empty:
            continue
        tok, idx, _, _, _, st = W.sample_pool_host(pid, bits, params[r], P.java_random_state(seed))
        assert (int(toks[r]), int(idxs[r]), int(states[r])) == (tok, idx, st), name
