"""-m gpu: the three list kernels of the device-routed MoE layer alone (ifa_moe_build_lists, ifa_moe_gather, ifa_moe_combine) on routings the
test decides, bit for bit against tests/moe_lists_util.py: every list over its counted records, every byte behind them and in a guard region
past the planned capacity still the sentinel.  tests/test_moe_lists_ref_cpu.py shows on the host that the comparison called here rejects every
fault of docs/moe_layer_edges.md for every case run here."""
import numpy as np
import pytest
import torch

import inferflow_amd as ia
from tests import gpu_util as g
from tests import moe_lists_util as M

pytestmark = pytest.mark.gpu


def _sentinel(nbytes):
    return torch.full((nbytes,), M.SENTINEL, dtype=torch.uint8, device="cuda")


def _build(c, sel, wsel):
    caps = M.capacities(c.T, c.top_k, c.E, c.tile_rows)
    out = {k: _sentinel(M.raw_bytes(caps, k)) for k in M.KEYS}
    ia.check(g.capi().ifa_moe_build_lists(g.p(g.dev(sel)), g.p(g.dev(wsel)), c.T, c.top_k, c.E, c.tile_rows, c.small_max, g.p(out["idx"]), g.p(out["wdev"]),
                                          g.p(out["epos"]), g.p(out["tiles"]), g.p(out["singles"]), g.p(out["smalls"]), g.p(out["counts"]), g.stream()))
    g.sync()
    return out, caps


@pytest.mark.parametrize("c", M.CASES, ids=[c.id for c in M.CASES])
def test_build_lists(c):
    sel, wsel = M.make_routing(c)
    want = M.build_lists(sel, wsel, c.T, c.top_k, c.E, c.tile_rows, c.small_max)
    out, caps = _build(c, sel, wsel)
    M.compare_lists({k: v.cpu().numpy() for k, v in out.items()}, want, caps)


def test_build_lists_twice_into_the_same_arrays():
    """a second routing with fewer entries into arrays the first one filled: counts and epos are rewritten, nothing of the first launch is read"""
    big, small = M.Case(8, 2, 1024, 64, 8, "uniform"), M.Case(8, 2, 1024, 64, 8, "holes")
    caps = M.capacities(big.T, big.top_k, big.E, big.tile_rows)
    out = {k: _sentinel(M.raw_bytes(caps, k)) for k in M.KEYS}
    for c in (big, small):
        sel, wsel = M.make_routing(c)
        ia.check(g.capi().ifa_moe_build_lists(g.p(g.dev(sel)), g.p(g.dev(wsel)), c.T, c.top_k, c.E, c.tile_rows, c.small_max, g.p(out["idx"]),
                                              g.p(out["wdev"]), g.p(out["epos"]), g.p(out["tiles"]), g.p(out["singles"]), g.p(out["smalls"]),
                                              g.p(out["counts"]), g.stream()))
        g.sync()
        want = M.build_lists(sel, wsel, c.T, c.top_k, c.E, c.tile_rows, c.small_max)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        if c is big:
            M.compare_lists(got, want, caps)
            first = got
        else:       # the records behind the second launch's counts are the first launch's, byte for byte
            assert got["counts"][:16].view(np.int32).tolist() == want.counts.tolist()
            for k in M.KEYS:
                rec = np.ascontiguousarray(getattr(want, k), M.DTYPE[k]).reshape(-1)
                assert np.array_equal(got[k][:rec.nbytes].view(M.DTYPE[k]), rec), k
                assert np.array_equal(got[k][rec.nbytes:], first[k][rec.nbytes:]), (k, "bytes past the second launch's records changed")


def _lists_on_device(c):
    sel, wsel = M.rows_routing(c)
    lc = M.Case(c.E, c.top_k, c.T * c.top_k, 64, 8, "uniform")
    out, caps = _build(lc, sel, wsel)
    want = M.build_lists(sel, wsel, c.T, c.top_k, c.E, 64, 8)
    M.compare_lists({k: v.cpu().numpy() for k, v in out.items()}, want, caps)
    return sel, wsel, out, want


@pytest.mark.parametrize("c", M.GATHER_CASES, ids=[c.id for c in M.GATHER_CASES])
def test_gather(c):
    """max_entries (the grid) is the capacity, counts[0] less: the rows past counts[0] and the guard rows keep the sentinel"""
    sel, wsel, out, L = _lists_on_device(c)
    n, cap = int(L.counts[0]), c.T * c.top_k
    assert 0 < n < cap
    src = M.rows_data(c, c.T, 3)
    dst = _sentinel((cap + 2) * c.dim * 2)
    ia.check(g.capi().ifa_moe_gather(g.p(g.dev(src)), g.p(out["idx"]), g.p(out["counts"]), cap, c.dim, g.p(dst), g.stream()))
    g.sync()
    got = dst.cpu().numpy().view(np.uint16).reshape(cap + 2, c.dim)
    want = np.full((cap + 2, c.dim), M.SENTINEL * 0x0101, np.uint16)
    want[:n] = src[L.idx].view(np.uint16)
    M.compare_rows(got, want, "gathered rows")


@pytest.mark.parametrize("c", M.COMBINE_CASES, ids=[c.id for c in M.COMBINE_CASES])
def test_combine(c):
    sel, wsel, out, L = _lists_on_device(c)
    n = int(L.counts[0])
    y = M.rows_data(c, n, 1)
    res = M.rows_data(c, c.T, 2) if c.residual else None
    dst = _sentinel((c.T + 2) * c.dim * 2)
    ia.check(g.capi().ifa_moe_combine(g.p(g.dev(y)), g.p(out["epos"]), g.p(g.dev(wsel)), c.T, c.top_k, c.dim, g.p(g.dev(res)) if c.residual else None,
                                      g.p(dst), g.stream()))
    g.sync()
    got = dst.cpu().numpy().view(np.uint16).reshape(c.T + 2, c.dim)
    want = np.full((c.T + 2, c.dim), M.SENTINEL * 0x0101, np.uint16)
    want[:c.T] = M.combine(y, L.epos, wsel, res).view(np.uint16)
    M.compare_rows(got, want, "combined rows")
