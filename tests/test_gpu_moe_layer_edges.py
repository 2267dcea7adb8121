"""-m gpu: the device-routed mixture-of-experts layer on routings the test designs (tests/moe_layer_util.py, docs/moe_layer_edges.md), every
launch judged from the inputs the DEVICE had.  One case: a one-layer model (dim 256, 8 or 4 experts Q4_B32T1A N(0, 0.055) quantised on the device,
top 2, rope_order 0, Wv = Wo = 0 so that the FFN input of row i is embedding row i, whose first E columns are the code of the row's routing).
Before any number is compared the plan of the step must be the one the case is designed for.  Then
  router   rows_a = the embedding rows (bytes); rows_hn within one F16 ulp of the oracle's norm; moe_gate within 4 ulps of the float64 softmax of
           G x hn; moe_sel = the designed routing; moe_sel / moe_selw = oracle.moe_topk of the read-back moe_gate (bytes)
  lists    moe_counts and every list = build_lists(moe_sel, moe_selw) (tests/moe_lists_util.py); moe_gin = rows_hn[moe_idx] (bytes)
  products per list (tiles, smalls, singles): gated moe_g1 and moe_g3 from moe_gin, moe_gout from moe_g1, within max(2 x d_ref, one F16 ulp)
  combine  the step's output rows = combine(moe_gout, moe_epos, moe_selw, rows_a) (bytes)
tests/test_moe_layer_ref_cpu.py shows on the host that these assertions reject every fault of the document on these cases' own lists."""
import numpy as np
import pytest
import torch

from inferflow_amd import dtypes as dt, synth, worker as W
from tests import moe_layer_util as U
from tests import moe_lists_util as M
from tests import rows_gemm_util as R
from tests.decode_attn_util import ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTIONS = ("moe_singles", "rows_mo", "moe_overlap", "moe_router_fused")


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float16).view(np.int16)).to(DEV).view(torch.float16)


def _build(rc):
    D = rc.dim
    s = dict(dim=D, layers=1, heads=8, kv_heads=8, head_dim=32, ffn=rc.ffn, vocab=rc.V, experts=rc.E, moe_top_k=rc.K)
    wk = W.DecodeWorker(max_ctx=max(4, rc.n if rc.mode == "prompt" else 4), kv_dtype=dt.F16, rope_order=0, **s)
    Em = U.embedding(rc)
    wk.set_tensor_f16(-1, W.T_EMBD, dt.F16, _dev16(Em))
    wk.set_tensor_f16(-1, W.T_OUT_NORM, dt.F16, torch.ones(D, dtype=torch.float16, device=DEV))
    wk.set_tensor_f16(-1, W.T_LM_HEAD, dt.F16, synth.gen_f16((rc.V, D), 998, U.W_STD, DEV))
    wk.set_tensor_f16(0, W.T_ATTN_NORM, dt.F16, _dev16(R.norm_weight(D)))
    wk.set_tensor_f16(0, W.T_FFN_NORM, dt.F16, _dev16(U.ffn_norm_weight(rc.E, D)))
    for tid in (W.T_WQ, W.T_WK, W.T_WV, W.T_WO):
        rows, cols = (D, 256) if tid == W.T_WO else (256, D)      # (heads x head_dim = 256 whatever dim)
        t16 = synth.gen_f16((rows, cols), 1000 + tid, U.W_STD, DEV)
        if tid in (W.T_WV, W.T_WO):
            t16.zero_()                                  # the attention half adds exactly 0
        wk.set_tensor_f16(0, tid, U.WD, t16, rows, cols)
    for e in range(rc.E):
        for which, (rows, cols) in ((0, (rc.ffn, D)), (1, (rc.ffn, D)), (2, (D, rc.ffn))):
            wk.set_tensor_f16(0, U.T_OF[which], U.WD, synth.gen_f16((rows, cols), 100000 + 16 * e + which, U.W_STD, DEV), rows, cols, expert=e)
    wk.set_tensor_f16(0, W.T_MOE_GATE, dt.F16, _dev16(U.gate_weight(rc.E, D)))
    wk.finalize()
    if rc.mode == "batch":
        wk.kv_slots(rc.V)
    return wk, Em


def _tensors(wk, rc):
    out = {("e", e, w): wk.get_expert_tensor_host(0, e, U.T_OF[w]) for e in range(rc.E) for w in range(3)}
    out["gate"] = wk.get_tensor_host(0, W.T_MOE_GATE)
    out["embd"] = wk.get_tensor_host(-1, W.T_EMBD)
    return out


def _same_tensors(a, b):
    for k in a:
        assert np.array_equal(a[k][1], b[k][1]), ("a tensor changed", k)


def _run(wk, rc):
    n = rc.n
    if rc.mode == "batch":
        lg = torch.empty((n, rc.V), dtype=torch.float16, device=DEV)
        wk.decode_batch(np.arange(n), np.zeros(n), np.arange(n), lg)
    else:
        wk.forward(np.arange(n), 0)


def _read(wk, rc):
    n, K, E, D, F = rc.n, rc.K, rc.E, rc.dim, rc.ffn
    rd = lambda name, t: wk.read_buffer(name).view(t)
    b = dict(a=rd("rows_a", np.float16).reshape(-1, D)[:n], hn=rd("rows_hn", np.float16).reshape(-1, D)[:n], x=rd("rows_x", np.float16).reshape(-1, D)[:n],
             gate=rd("moe_gate", np.float16).reshape(-1, E)[:n], sel=rd("moe_sel", np.int32)[:n * K].reshape(n, K), selw=rd("moe_selw", np.float16)[:n * K].reshape(n, K),
             counts=rd("moe_counts", np.int32)[:4], idx=rd("moe_idx", np.int32), wdev=rd("moe_wdev", np.uint16), epos=rd("moe_epos", np.int32)[:n * K],
             tiles=rd("moe_tiles", np.int32), singles=rd("moe_singles", np.int32), smalls=rd("moe_smalls", np.int32),
             gin=rd("moe_gin", np.float16).reshape(-1, D), g1=rd("moe_g1", np.float16).reshape(-1, F), g3=rd("moe_g3", np.float16).reshape(-1, F),
             gout=rd("moe_gout", np.float16).reshape(-1, D))
    return b


class Stats:
    def __init__(self):
        self.worst, self.failed = {}, []

    def add(self, where, name, out16, ref):
        try:
            med, worst = U.check_launch(out16, ref)
        except AssertionError as e:                        # (every launch of the step is measured before the test fails)
            self.failed.append("%s: %s" % (where, e))
            return
        if worst > self.worst.get(name, (-1.0, ""))[0]:
            self.worst[name] = (worst, where)

    def report(self, title):
        for name, (w, where) in sorted(self.worst.items()):
            print("moe-layer-edges %-44s %-14s worst err / bound %.3f (%s)" % (title, name, w, where))
        assert not self.failed, "%d launches of %s: %s" % (len(self.failed), title, " | ".join(self.failed))


def _check(wk, rc, Em, experts, plan, stats, where):
    """everything of one step, from what the device left; returns the buffers"""
    n, K, E = rc.n, rc.K, rc.E
    b = _read(wk, rc)
    # -- router
    M.compare_rows(b["a"], Em[:n], where + ": rows_a against the embedding rows (the attention half must add exactly 0)")
    hn_orc = R.normed(b["a"], U.ffn_norm_weight(E, rc.dim))
    assert (np.abs(b["hn"].astype(np.float64) - hn_orc.astype(np.float64)) <= ulp16(hn_orc)).all(), (where, "rows_hn")
    lg = U.G_GATE * b["hn"][:, :E].astype(np.float64)
    ex = np.exp(lg - lg.max(axis=1, keepdims=True)); p64 = ex / ex.sum(axis=1, keepdims=True)
    assert (np.abs(b["gate"].astype(np.float64) - p64) <= 4 * ulp16(p64) + 2.0 ** -24).all(), (where, "moe_gate against the float64 softmax")
    assert np.array_equal(b["sel"], rc.sel()), (where, "moe_sel is not the designed routing", b["sel"].tolist(), rc.sel().tolist())
    sel_o, w_o = U.route_of_probs(b["gate"], K)
    assert np.array_equal(b["sel"], sel_o), (where, "moe_sel against oracle.moe_topk of moe_gate")
    M.compare_rows(b["selw"], w_o, where + ": moe_selw against oracle.moe_topk of moe_gate")
    # -- lists
    L = M.build_lists(b["sel"], b["selw"], n, K, E, plan["tile_rows"], plan["small_max"])
    M.compare_counted(b, L, n, K)
    c0 = int(L.counts[0])
    assert len(L.tiles) <= plan["max_tiles"] and len(L.singles) <= plan["max_singles"] and len(L.smalls) <= plan["max_smalls"], (where, L.counts, plan)
    M.compare_rows(b["gin"][:c0], b["hn"][L.idx], where + ": moe_gin against the gathered rows")
    # -- products
    ref = U.LayerRef(experts, L, b["gin"], b["g1"])
    grouped = plan["kind"] == "device_grouped"
    for name, lr in ref.launches().items():
        kind, buf = name.split(".")
        if buf == "g3" and not (grouped and (kind != "smalls" or not plan["smalls_mo"])):
            continue                                     # (the singles route and the MO small groups gate their own product: g3 is not written)
        stats.add(where, name, b[buf][lr.rows], lr)
    # -- combine
    M.compare_rows(b["x"], M.combine(b["gout"][:c0], L.epos, b["selw"], b["a"]), where + ": output rows against combine(moe_gout)")
    b["L"] = L
    return b


def _set_options(wk, opts):
    for k in OPTIONS:
        wk.set_option(k, opts.get(k, 1))


def _experts_of(wk, rc):
    raw = _tensors(wk, rc)
    return raw, [U.Expert({w: raw[("e", e, w)] for w in range(3)}) for e in range(rc.E)]


BATCH = U.batch_singles_cases() + U.batch_grouped_cases() + [c for c in U.tie_cases() if c.mode == "batch"] + U.router_cases()
PROMPT = U.prompt_cases() + [c for c in U.tie_cases() if c.mode == "prompt"]


@pytest.mark.parametrize("rc", BATCH, ids=[c.id for c in BATCH])
def test_every_launch_of_a_batched_step(rc):
    wk, Em = _build(rc)
    raw, experts = _experts_of(wk, rc)
    stats = Stats()
    got = {}
    sets = U.OPTION_SETS if rc.n <= 8 and rc.name != "router" else (U.OPTION_SETS[0], U.OPTION_SETS[4])
    for name, opts in sets:
        _set_options(wk, opts)
        _run(wk, rc)
        plan = wk.moe_plan(0, rc.n, caller_norm=1)
        want = U.expected_plan(rc, opts)
        if rc.dim != U.DIM:                              # (which launches serve a 4096-column expert is the launchers' business: the router is this case's subject)
            assert plan["router"] == want["router"] and plan["kind"] != "host", (rc.id, name, plan)
        else:
            assert {k: plan[k] for k in U.PLAN_KEYS} == want, (rc.id, name, plan)
        got[name] = _check(wk, rc, Em, experts, plan, stats, "%s %s" % (rc.id, name))
    d = got["default"]
    # the one-launch router against the four launches: the same bytes
    for k in ("gate", "sel", "selw", "hn"):
        assert np.array_equal(d[k].view(np.uint16 if d[k].dtype == np.float16 else d[k].dtype), got["router_ops"][k].view(np.uint16 if d[k].dtype == np.float16 else d[k].dtype)), (rc.id, k, "fused router against the four launches")
    # the singles route against the grouped int8 GEMV on the singles' rows of moe_gout (csrc/ifa_decode_singles.h): the same bytes
    if "moe_singles0" in got and len(d["L"].singles):
        pos = d["L"].singles[:, 1]
        M.compare_rows(d["gout"][pos], got["moe_singles0"]["gout"][pos], rc.id + ": singles route against the grouped GEMV route")
        M.compare_rows(d["g1"][pos], got["moe_singles0"]["g1"][pos], rc.id + ": gated rows, singles route against the grouped GEMV route")
    for name in got:                                     # whatever launches ran, the same lists and the same output bytes where the arithmetic is the same
        assert got[name]["L"].counts.tolist() == d["L"].counts.tolist()
    M.compare_rows(got["moe_overlap0"]["x"], d["x"], rc.id + ": without the side stream") if "moe_overlap0" in got else None
    _same_tensors(raw, _tensors(wk, rc))
    wk.close()
    stats.report(rc.id)


@pytest.mark.parametrize("rc", PROMPT, ids=[c.id for c in PROMPT])
def test_every_launch_of_a_prompt(rc):
    wk, Em = _build(rc)
    raw, experts = _experts_of(wk, rc)
    stats = Stats()
    _run(wk, rc)
    plan = wk.moe_plan(0, rc.n)
    have_mo = plan["smalls_mo"] if plan["small_max"] else 1      # (whether the prompt route built the MO copies is the prompt route's business)
    assert {k: plan[k] for k in U.PLAN_KEYS} == U.expected_plan(rc, None, have_mo), (rc.id, plan)
    b = _check(wk, rc, Em, experts, plan, stats, rc.id)
    if rc.name == "first0" and rc.n >= 33:
        rows = b["L"].tiles[b["L"].tiles[:, 0] == 0][:, 2].tolist()
        assert rows == {33: [33], 65: [64, 1], 129: [64, 64, 1], 193: [128, 65]}[rc.n], rows
    _same_tensors(raw, _tensors(wk, rc))
    wk.close()
    stats.report(rc.id)


# ----------------------------------------------------------------------------- order effects
def _vocab():
    """32 embedding rows of mixed routing: 0-7 the groups routing of 8 rows, 8-15 one expert each (dropped slot), 16-23 all on experts 0 and 1, 24-31 ties"""
    g = U.from_counts("groups", "batch", 8, 2, 8, [1, 5, 1, 3, 2, 4]).rows
    t = [c for c in U.tie_cases() if c.mode == "batch"][0].rows
    return U.Routing("vocab", "batch", 8, 2, g + [U.only(e) for e in range(8)] + [U.pair(0, 1) if i % 2 else U.pair(1, 0) for i in range(8)] + t)


def _sub(voc, toks):
    return U.Routing("sub", "batch", voc.E, voc.K, [voc.rows[t] for t in toks])


def _step(wk, toks, logits=True):
    n = len(toks)
    lg = torch.empty((n, 32), dtype=torch.float16, device=DEV) if logits else None
    wk.decode_batch(np.asarray(toks), np.zeros(n), np.arange(n), lg)


SENT = ("moe_gin", "moe_gout", "moe_g1", "moe_idx", "moe_wdev", "moe_tiles", "moe_singles", "moe_smalls", "moe_epos", "moe_sel", "moe_selw")


def test_a_small_step_behind_a_large_one_leaves_the_rest_of_the_buffers_alone():
    """the largest step first, then a sentinel over the gathered rows, the outputs and the lists; a 2-row step behind it must leave every row past
    its counts[0] and every record past its counts untouched (singles route: moe_g1 too -- on the grouped route the element-wise and quantiser
    launches run over all `cap` rows by design, docs/moe_layer_edges.md)"""
    voc = _vocab()
    wk, Em = _build(voc)
    raw, experts = _experts_of(wk, voc)
    big, small = list(range(8)), [3, 8]                      # 16 entries, then 3 (a pair and a row with a dropped slot)
    _step(wk, big)
    for name in SENT:
        p, nb = wk.buffer(name)
        wk.write_buffer(name, np.full(nb, M.SENTINEL, np.uint8))
    _step(wk, small)
    rc = _sub(voc, small)
    plan = wk.moe_plan(0, 2, caller_norm=1)
    assert plan["kind"] == "device_singles", plan
    stats = Stats()
    b = _check(wk, rc, Em[small], experts, plan, stats, "2 rows behind 8")
    L = b["L"]
    c0, nt, ns, nm = (int(v) for v in L.counts)
    assert c0 == 3
    D, F = voc.dim, voc.ffn
    keep = dict(moe_gin=c0 * D * 2, moe_gout=c0 * D * 2, moe_g1=c0 * F * 2, moe_idx=c0 * 4, moe_wdev=c0 * 2, moe_tiles=nt * 16, moe_singles=ns * 8, moe_smalls=nm * 16,
                moe_epos=2 * 2 * 4, moe_sel=2 * 2 * 4, moe_selw=2 * 2 * 2)
    for name, used in keep.items():
        rest = wk.read_buffer(name)[used:]
        assert rest.size and (rest == M.SENTINEL).all(), "%s: byte %d past the step's %d bytes was written" % (name, int(np.flatnonzero(rest != M.SENTINEL)[0]), used)
    _same_tensors(raw, _tensors(wk, voc))
    wk.close()
    stats.report("2 rows behind 8")


def test_a_captured_step_replayed_on_another_routing_rebuilds_its_lists():
    """a batched step captured on one routing (two groups of 8 rows, no single) and replayed with tokens of another (other counts, groups that
    become singles, dropped slots) must leave what the eager step of those tokens leaves, byte for byte: the lists are rebuilt on the device
    inside the graph, every launch reads its counts there"""
    voc = _vocab()
    wk, Em = _build(voc)
    raw, experts = _experts_of(wk, voc)
    A, B = list(range(16, 24)), [0, 1, 2, 3, 8, 9, 10, 27]
    names = ("rows_x", "moe_counts", "moe_sel", "moe_selw", "moe_epos", "moe_idx", "moe_wdev", "moe_singles", "moe_smalls")
    rcB = _sub(voc, B)
    plan = None
    stats = Stats()
    _step(wk, B)                                             # eager
    plan = wk.moe_plan(0, 8, caller_norm=1)
    eager = _check(wk, rcB, Em[B], experts, plan, stats, "eager")
    c0, nt, ns, nm = (int(v) for v in eager["L"].counts)
    assert (c0, nt) == (int(rcB.counts().sum()), 0) and ns >= 2 and nm >= 1 and c0 < 16
    W.gemm_rows_launches()
    _step(wk, A, logits=False)                               # captured, run once
    cA = wk.read_buffer("moe_counts").view(np.int32)[:4].tolist()
    assert cA == [16, 0, 0, 2], cA
    assert W.gemm_rows_launches()[1] > 0, "the capture records the launches of its attention half"
    _step(wk, A, logits=False)                               # replayed
    _step(wk, B, logits=False)                               # replayed on the other routing
    assert W.gemm_rows_launches()[1] == 0, "the two steps behind the capture are replays: no launch from the host"
    replay = _check(wk, rcB, Em[B], experts, plan, stats, "replay")
    for k in ("x", "gate", "sel", "selw", "hn", "epos"):
        assert np.array_equal(np.ascontiguousarray(eager[k]).view(np.uint8), np.ascontiguousarray(replay[k]).view(np.uint8)), (k, "replay against eager")
    for k, used in (("gin", c0), ("g1", c0), ("gout", c0), ("idx", c0), ("wdev", c0), ("singles", 2 * ns), ("smalls", 4 * nm)):
        assert np.array_equal(np.ascontiguousarray(eager[k][:used]).view(np.uint8), np.ascontiguousarray(replay[k][:used]).view(np.uint8)), (k, "replay against eager")
    _same_tensors(raw, _tensors(wk, voc))
    wk.close()
    stats.report("captured step replayed")
