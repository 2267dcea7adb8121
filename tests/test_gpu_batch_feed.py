"""-m gpu: the feed kernel (csrc/ifa_batch_feed.hip, ifa_batch_feed_rows) against the same rule compiled for the host
(ifa_batch_feed_host, itself pinned to its specification by tests/test_batch_feed_cpu.py) on that test's cases: every array the
feed reads or writes, byte for byte, after each of the consecutive launches on the same device state.  Then the counts clamp."""
import numpy as np
import pytest

from inferflow_amd import worker as W
from tests import batch_feed_util as U

pytestmark = pytest.mark.gpu

CASES = U.cases()


def _to_dev(A):
    import torch
    out = {}
    for k, v in A.items():
        if v is None:
            out[k] = None
        elif v.dtype in (W.BATCH_FEED_ROW, W.BATCH_ATTN_ROW):
            out[k] = torch.from_numpy(v.copy().view(np.uint8).reshape(-1)).cuda()
        elif v.dtype == np.uint64:
            out[k] = torch.from_numpy(v.view(np.int64).copy()).cuda()
        else:
            out[k] = torch.from_numpy(v.copy()).cuda()
    return out


def _to_host(D, like):
    out = {}
    for k, v in like.items():
        out[k] = None if v is None else D[k].cpu().numpy().view(v.dtype).reshape(v.shape)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_host_rule_over_consecutive_launches(case):
    import torch
    _, n, layers, A, inputs = case
    assert len(inputs) >= 3
    host = U.clone(A)
    dev = _to_dev(A)
    for s, inp in enumerate(inputs):
        U.load_inputs(host, inp)
        for name, v in inp.items():
            dev[name].copy_(torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v))
        W.batch_feed_host(n, layers, host)
        W.batch_feed_rows(n, layers, dev)
        torch.cuda.synchronize()
        U.assert_same(_to_host(dev, host), host, "launch %d" % s)


def test_launches_queue_up_without_the_host_between_them():
    """the step number comes from device memory: three launches enqueued back to back on unchanged inputs are three steps"""
    import torch
    _, n, layers, A, inputs = CASES[0]
    host = U.clone(A)
    U.load_inputs(host, inputs[0])
    dev = _to_dev(host)
    for _ in range(3):
        W.batch_feed_host(n, layers, host)
        W.batch_feed_rows(n, layers, dev)
    torch.cuda.synchronize()
    assert int(host["step"][0]) == 3
    U.assert_same(_to_host(dev, host), host, "three launches")


def test_clamp_counts():
    import torch
    g = np.random.RandomState(5)
    for rows in (1, 2, 32, 64, 65, 200):
        counts = g.randint(0, 257, rows).astype(np.int32)
        pool_len = g.randint(1, 257, rows).astype(np.int32)
        c = torch.from_numpy(counts).cuda()
        W.batch_clamp_counts(c, torch.from_numpy(pool_len).cuda())
        assert np.array_equal(c.cpu().numpy(), np.minimum(counts, pool_len)), rows
