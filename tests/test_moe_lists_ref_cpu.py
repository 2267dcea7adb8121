"""No GPU: the numpy restatement of the MoE list kernels (tests/moe_lists_util.py) against the reference's own selections, the cases of
tests/test_gpu_moe_lists.py against what the issue's list asks of them, the fault list -- every fault applied to the reference output of
every device case must be rejected by the comparison the GPU test calls -- and the refusals of the three entry points, which happen before
any launch."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import moe_lists_util as M

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_moe_rows.npz")
Z = np.load(FIX)
META = json.loads(bytes(Z["meta"]).decode())


# ----------------------------------------------------------------------------- the reference against the reference's selections
@pytest.mark.parametrize("i", range(len(META)))
def test_lists_hold_each_experts_rows_in_the_references_order(i):
    """The reference keeps, per row, (expert, weight) items (BuildRowsForMoE) and then walks the experts in ascending id, each over the rows in
    token order (ProcessGpuLayer_Moe's expert loop).  Those per-expert row and weight lists, built here directly from its recorded items, must be
    what build_lists leaves in idx / wdev between an expert's first and last entry -- from the routers' form of the same selection (a row's
    experts ascending, -1 behind them)."""
    m, probs, n_ref, e_ref, w_ref = META[i], Z["c%d_probs" % i], Z["c%d_n" % i], Z["c%d_e" % i], Z["c%d_w" % i]
    T, E = probs.shape
    K = min(m["top_k"], 8)
    rows, wts = [[] for _ in range(E)], [[] for _ in range(E)]
    sel = np.full((T, K), -1, np.int32)
    wsel = np.zeros((T, K), np.float16)
    for t in range(T):
        n = int(n_ref[t])
        for j in range(n):
            rows[int(e_ref[t][j])].append(t); wts[int(e_ref[t][j])].append(np.float16(w_ref[t][j]))
        order = np.argsort(e_ref[t][:n], kind="stable")
        sel[t, :n] = e_ref[t][:n][order]; wsel[t, :n] = w_ref[t][:n][order].astype(np.float16)
    for tile_rows, small_max in ((64, 0), (64, 8), (128, 8)):
        L = M.build_lists(sel, wsel, T, K, E, tile_rows, small_max)
        off = 0
        for e in range(E):
            c = len(rows[e])
            assert L.idx[off:off + c].tolist() == rows[e], (e, "rows")
            assert L.wdev[off:off + c].tolist() == [int(np.float16(w).view(np.uint16)) for w in wts[e]], (e, "weights")
            kinds = [("single", r) for r in L.singles if r[0] == e] + [("small", r) for r in L.smalls if r[0] == e] + [("tile", r) for r in L.tiles if r[0] == e]
            if c == 0:
                assert not kinds
            elif c == 1:
                assert [k for k, _ in kinds] == ["single"] and kinds[0][1][1] == off
            elif c <= small_max:
                assert [k for k, _ in kinds] == ["small"] and kinds[0][1].tolist() == [e, off, c, 0]
            else:
                assert [k for k, _ in kinds] == ["tile"] * -(-c // tile_rows)
                assert [int(r[1]) for _, r in kinds] == list(range(off, off + c, tile_rows)) and sum(int(r[2]) for _, r in kinds) == c
                assert all(1 <= int(r[2]) <= tile_rows and r[3] == 0 for _, r in kinds)
            off += c
        assert L.counts.tolist() == [off, len(L.tiles), len(L.singles), len(L.smalls)]
        live = sel.reshape(-1) >= 0
        assert (L.epos[~live] == -1).all() and sorted(L.epos[live].tolist()) == list(range(off))
        assert np.array_equal(L.idx[L.epos[live]], np.flatnonzero(live) // K)
        # the lists are sorted by expert (tiles: then by row) -- the order the header states
        for a in (L.tiles, L.singles, L.smalls):
            assert [tuple(r[:2]) for r in a] == sorted(tuple(r[:2]) for r in a)


def test_hfma_rounds_once():
    """against exact rational arithmetic, on operands whose float64 sum is inexact (65504 + a product of subnormals) and on ties"""
    rng = np.random.default_rng(3)
    a = rng.normal(0, 1, 4000).astype(np.float16)
    w = rng.uniform(0, 1, 4000).astype(np.float16)
    c = rng.normal(0, 1, 4000).astype(np.float16)
    a[:6] = np.array([6e-8, -6e-8, 1.0, 3.0, 1.0009765625, 60000.0], np.float16)
    w[:6] = np.array([6e-8, 6e-8, 2.0 ** -11, 2.0 ** -12, 1.0009765625, 1.0], np.float16)
    c[:6] = np.array([65504.0, 2048.0, 1.0, 1.0, -1.0, 60000.0], np.float16)
    got = M.hfma(a, w, c)

    def to_half(q):                                         # round to nearest even from an exact rational
        if q == 0:
            return np.float16(0)
        s, q = (-1, -q) if q < 0 else (1, q)
        e = max(-14, int(np.floor(np.log2(float(q)))))
        while Fraction(2) ** e > q and e > -14:
            e -= 1
        while Fraction(2) ** (e + 1) <= q:
            e += 1
        ulp = Fraction(2) ** (e - 10)
        n = q / ulp
        f = n.numerator // n.denominator
        r = n - f
        if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
            f += 1
        v = float(f * ulp)
        return np.float16(s * v) if v <= 65504 else np.float16(s * np.inf)

    with np.errstate(over="ignore"):
        for i in list(range(64)) + list(range(3000, 3040)):
            want = to_half(Fraction(float(a[i])) * Fraction(float(w[i])) + Fraction(float(c[i])))
            assert got[i].view(np.uint16) == want.view(np.uint16), (i, a[i], w[i], c[i], got[i], want)


# ----------------------------------------------------------------------------- the cases are the ones asked for
def test_cases_cover_every_value_and_every_count_edge_per_list_kind():
    cs = M.CASES
    assert 24 <= len(cs) <= 48 and len({c.id for c in cs}) == len(cs)
    assert {c.E for c in cs} == {1, 4, 8, 63, 64} and {c.top_k for c in cs} == {1, 2, 8} and all(c.top_k <= c.E for c in cs)
    assert {c.N for c in cs} == {1, 63, 64, 65, 1023, 1024, 1025, 2400} and all(c.N % c.top_k == 0 for c in cs)
    assert {(c.tile_rows, c.small_max) for c in cs} == {(64, 0), (64, 8), (128, 8)}
    assert {c.family for c in cs} == {"uniform", "all0", "alllast", "forced", "forced_hi", "holes"}
    seen = set()                                            # (tile_rows, small_max, rows of an expert, list kind)
    for c in cs:
        sel, wsel = M.make_routing(c)
        assert sel.shape == (c.T, c.top_k) and wsel.shape == sel.shape and wsel.dtype == np.float16
        for t in range(c.T):
            live = sel[t][(sel[t] >= 0) & (sel[t] < c.E)]
            assert len(set(live.tolist())) == len(live), "an expert twice in a row"
        L = M.build_lists(sel, wsel, c.T, c.top_k, c.E, c.tile_rows, c.small_max)
        kind = {int(r[0]): "single" for r in L.singles}
        kind.update({int(r[0]): "small" for r in L.smalls}); kind.update({int(r[0]): "tile" for r in L.tiles})
        cnt = np.bincount(sel[(sel >= 0) & (sel < c.E)].reshape(-1), minlength=c.E)
        if c.family in ("forced", "forced_hi"):
            assert cnt.tolist() == M.forced_counts(c), c.id
        if c.family == "all0":
            assert cnt[0] == c.T and cnt.sum() == c.T
        if c.family == "alllast":
            assert cnt[c.E - 1] == c.T and cnt.sum() == c.T
        if c.family == "holes":
            assert 0.2 < (L.counts[0] / c.N if c.N > 8 else 0.3) < 0.85
        for e in range(c.E):
            seen.add((c.tile_rows, c.small_max, int(cnt[e]), kind.get(e, "none")))
        caps = M.capacities(c.T, c.top_k, c.E, c.tile_rows)
        assert all(L.counts[i] <= caps[k] for i, k in enumerate(("idx", "tiles", "singles", "smalls"))), (c.id, L.counts, caps)
    for tr, sm in ((64, 0), (64, 8), (128, 8)):
        for n in M.count_edges(tr, sm):
            want = "none" if n == 0 else "single" if n == 1 else "small" if n <= sm else "tile"
            assert (tr, sm, n, want) in seen, "no case gives an expert %d rows (%s) at tile_rows %d, small_max %d" % (n, want, tr, sm)
    # the list capacities themselves are reached: singles = E, smalls = min(E, cap / 2)
    c = M.Case(64, 8, 64, 64, 8, "uniform")
    assert c in cs


# ----------------------------------------------------------------------------- the faults
@pytest.mark.parametrize("c", M.CASES, ids=[c.id for c in M.CASES])
def test_the_comparison_accepts_the_reference_and_rejects_every_fault(c):
    sel, wsel = M.make_routing(c)
    L = M.build_lists(sel, wsel, c.T, c.top_k, c.E, c.tile_rows, c.small_max)
    caps = M.capacities(c.T, c.top_k, c.E, c.tile_rows)
    M.compare_lists(M.as_device(L, caps), L, caps)
    faults = M.list_faults(L, sel, wsel, c)
    assert set(faults) <= set(M.LIST_FAULTS)
    for name, bad in faults.items():
        # (a fault may overflow the planned capacity -- one tile too many: lay it out with room, the comparison still has to see it)
        room = {k: max(v, len(np.asarray(getattr(bad, k)).reshape(-1)) // M.WIDTH[k]) for k, v in caps.items()}
        dev = M.as_device(bad, room)
        dev = {k: v[:M.raw_bytes(caps, k)] for k, v in dev.items()}
        with pytest.raises(AssertionError):
            M.compare_lists(dev, L, caps)
    # a write past the counted records, inside the capacity or in the guard
    for k in M.KEYS:
        for at in (-1, -M.GUARD * M.WIDTH[k] * np.dtype(M.DTYPE[k]).itemsize - 1):
            dev = M.as_device(L, caps)
            n_rec = np.asarray(getattr(L, k)).size * np.dtype(M.DTYPE[k]).itemsize
            if dev[k].size + at < n_rec:
                continue
            dev[k][at] = 0
            with pytest.raises(AssertionError):
                M.compare_lists(dev, L, caps)


def test_every_list_fault_is_shown_by_some_case_and_the_structural_ones_by_many():
    shown = {}
    for c in M.CASES:
        sel, wsel = M.make_routing(c)
        L = M.build_lists(sel, wsel, c.T, c.top_k, c.E, c.tile_rows, c.small_max)
        for name in M.list_faults(L, sel, wsel, c):
            shown[name] = shown.get(name, 0) + 1
    assert set(shown) == set(M.LIST_FAULTS), set(M.LIST_FAULTS) - set(shown)
    assert all(shown[n] >= 5 for n in M.LIST_FAULTS), shown


@pytest.mark.parametrize("c", M.COMBINE_CASES, ids=[c.id for c in M.COMBINE_CASES])
def test_combine_reference_and_its_faults(c):
    sel, wsel = M.rows_routing(c)
    L = M.build_lists(sel, wsel, c.T, c.top_k, c.E, 64, 8)
    assert L.counts[0] < c.T * c.top_k and (sel[c.T // 2] < 0).all()
    y = M.rows_data(c, int(L.counts[0]), 1)
    res = M.rows_data(c, c.T, 2) if c.residual else None
    want = M.combine(y, L.epos, wsel, res)
    # the definition, element by element in exact arithmetic on a sample
    ep = L.epos.reshape(c.T, c.top_k)
    for t in (0, c.T // 2, c.T - 1):
        for d in (0, 1, c.dim - 1):
            acc = np.float16(0)
            for j in range(c.top_k):
                if ep[t, j] >= 0:
                    acc = M.hfma(y[ep[t, j], d], wsel[t, j], acc)
            if res is not None:
                with np.errstate(over="ignore"):
                    acc = np.float16(np.float32(res[t, d]) + np.float32(acc))
            assert acc.view(np.uint16) == want[t, d].view(np.uint16), (t, d)
    assert not want[c.T // 2].any() if res is None else np.array_equal(want[c.T // 2].view(np.uint16), res[c.T // 2].view(np.uint16))
    M.compare_rows(want, want.copy(), "combine")
    faults = M.combine_faults(y, L.epos, wsel, res)
    assert set(faults) == (set(M.COMBINE_FAULTS) if c.residual else set())
    for name, bad in faults.items():
        with pytest.raises(AssertionError):
            M.compare_rows(bad, want, name)
    # the list faults that move no list the combine does not read must still move its rows: exchanged epos, a neighbour's weight
    if c.top_k > 1:
        lf = M.list_faults(L, sel, wsel, M.Case(c.E, c.top_k, c.T * c.top_k, 64, 8, "uniform"))
        bad = lf["epos of slots j and j + 1 exchanged"]
        with pytest.raises(AssertionError):
            M.compare_rows(M.combine(y, bad.epos, wsel, res), want, "epos exchanged")


# ----------------------------------------------------------------------------- the entry points refuse before they launch
def test_entry_points_refuse_what_the_kernels_cannot_take():
    import inferflow_amd as ia
    L = ia.lib()
    p = C.c_void_p(0x1000)                                  # never dereferenced: every call below must be refused on the host
    ok = dict(sel=p, wsel=p, tokens=4, top_k=2, experts=8, tile_rows=64, small_max=8, idx=p, wdev=p, epos=p, tiles=p, singles=p, smalls=p, counts=p)

    def build(**kw):
        a = dict(ok, **kw)
        return L.ifa_moe_build_lists(a["sel"], a["wsel"], a["tokens"], a["top_k"], a["experts"], a["tile_rows"], a["small_max"], a["idx"], a["wdev"],
                                     a["epos"], a["tiles"], a["singles"], a["smalls"], a["counts"], None)

    bad = [dict(experts=0), dict(experts=65), dict(experts=-1), dict(top_k=0), dict(top_k=9), dict(tile_rows=32), dict(tile_rows=96), dict(tile_rows=256),
           dict(tile_rows=0), dict(small_max=-1), dict(small_max=9)] + [{k: None} for k in ("sel", "wsel", "idx", "wdev", "epos", "tiles", "singles", "smalls", "counts")]
    for kw in bad:
        assert build(**kw) == -1, kw
        assert b"ifa_moe_build_lists" in L.ifa_last_error()
    for args in [(None, p, p, 4, 256, p), (p, None, p, 4, 256, p), (p, p, None, 4, 256, p), (p, p, p, 4, 256, None), (p, p, p, 4, 250, p), (p, p, p, 4, 0, p),
                 (p, p, p, 70000, 256, p), (C.c_void_p(0x1008), p, p, 4, 256, p)]:
        assert L.ifa_moe_gather(*args, None) == -1, args
        assert b"ifa_moe_gather" in L.ifa_last_error()
    for args in [(None, p, p, 4, 2, 256, None, p), (p, None, p, 4, 2, 256, None, p), (p, p, None, 4, 2, 256, None, p), (p, p, p, 4, 2, 256, None, None),
                 (p, p, p, 4, 0, 256, None, p), (p, p, p, 4, 9, 256, None, p), (p, p, p, 4, 2, 0, None, p), (p, p, p, 70000, 2, 256, None, p)]:
        assert L.ifa_moe_combine(*args, None) == -1, args
        assert b"ifa_moe_combine" in L.ifa_last_error()
