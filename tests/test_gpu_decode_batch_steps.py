"""-m gpu: the device-fed batched steps at the worker level (ifa_model_decode_batch_steps, csrc/ifa_engine_batch_steps.hip).  One call
of 6 steps against 6 one-step calls of the existing entry points from re-prefilled slots with the feed rule applied on the host:
ifa_model_decode_batch for batches of plain greedy rows, ifa_model_pool_adjust + ifa_model_decode_batch_pool + ifa_sample_pool_rows
on the pools (the device's exp on both sides) + ifa_model_logit_state_add otherwise.  Tokens, emitted counts, generator words, the
logit state and every K / V buffer are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import inferflow_amd as ia
from inferflow_amd import _capi, dtypes as dt, synth
from inferflow_amd import worker as W

pytestmark = pytest.mark.gpu

MAX_CTX, STEPS = 64, 6
# ragged contexts: 1, 5, 33 keys ...; row 3 ends on the last cache row (58 + 6 == 64)
CTX = [1, 5, 33, MAX_CTX - STEPS, 12, 2, 40, 7, 20, 3, 50, 9, 31, 32, 16, 4, 26]
BIAS = {17: -100.0, 400: float("-inf")}
TOP_P, MIN_P, GREEDY = (4, 0.9, 0.9, 8, 0.05), (7, 1.1, 0.9, 8, 0.05), (2, 1.0, 1.0, 1, 0.0)
B_FACTS = ("n", "exact_order", "may_chunk", "rows_mo", "gemm_rows", "batch_fused", "rows_kparts", "batch_graph", "graph", "topo", "rows_layers",
           "has_moe", "logits_out")
B_OUT = ("kind", "chunk", "norm_fused", "captured", "gm_kernel", "gm_src", "gm_mo", "gm_no_waits", "need_mo")


def _plan(n, has_moe=0):
    """ifa_batch_route_plan for a call of n rows on a Q4_B32T1A model with the default options"""
    f = dict(n=n, exact_order=0, may_chunk=1, rows_mo=1, gemm_rows=1, batch_fused=1, rows_kparts=1, batch_graph=0, graph=1, topo=0, rows_layers=2,
             has_moe=has_moe, logits_out=0)
    facts = (C.c_int * len(B_FACTS))(*[int(f[k]) for k in B_FACTS])
    out = (C.c_int * len(B_OUT))()
    ia.check(ia.lib().ifa_batch_route_plan(facts, len(B_FACTS), out, len(B_OUT)))
    return dict(zip(B_OUT, out))


def _one_fused_step(n, has_moe=0):
    p = _plan(n, has_moe)
    return p["kind"] == 2 and p["captured"] == 1 and p["chunk"] == 0


class Bed:
    """a worker with one prefilled KV slot per row"""

    def __init__(self, shape, kvd, n_slots):
        self.wk, _, self.s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=MAX_CTX, quant_threshold=0, std=0.06)
        self.V, self.layers, self.n_slots = self.s["vocab"], self.s["layers"], n_slots
        self.wk.kv_slots(n_slots)
        rng = np.random.default_rng(7)
        self.pos = np.array(CTX[:n_slots], np.int32)
        self.prompts = [rng.integers(3, self.V, int(p)).astype(np.int32) for p in self.pos]
        self.t0 = np.zeros(n_slots, np.int32)
        for sl in range(n_slots):
            self.wk.select_kv(sl)
            self.t0[sl] = self.wk.forward(self.prompts[sl], 0)
        self.wk.select_kv(0)
        self.snap = self.kv()
        self.armed = False

    def kv(self, n=None):
        out = []
        for sl in range(self.n_slots if n is None else n):
            self.wk.select_kv(sl)
            out.append([self.wk.read_buffer(name, l).copy() for l in range(self.layers) for name in ("kcache", "vcache")])
        self.wk.select_kv(0)
        return out

    def restore(self, n=None):
        """the slots as the prefill left them; the logit state of every slot: its prompt marked, its first token counted"""
        for sl in range(self.n_slots if n is None else n):
            self.wk.select_kv(sl)
            for i, b in enumerate(self.snap[sl]):
                self.wk.write_buffer(("kcache", "vcache")[i % 2], b, i // 2)
            if self.armed:
                self.wk.logit_state_reset(sl, self.prompts[sl], rep=1.3, freq=0.25, pres=0.5, bias={**BIAS, int(self.prompts[sl][0]): 5.0})
        self.wk.select_kv(0)
        if self.armed:
            k = self.n_slots if n is None else n
            self.wk.logit_state_add(list(range(k)), [int(t) for t in self.t0[:k]])
            self.wk.sync()

    def arm(self):
        self.armed = True

    def state(self):
        return self.wk.read_buffer("logit_state", nbytes=self.n_slots * self.V * 4).view(np.uint32).copy() if self.armed else None


_BEDS = {}


def _bed(shape, kvd, n_slots, armed=True):
    key = (shape, kvd)
    if key not in _BEDS or _BEDS[key].n_slots < n_slots:
        if key in _BEDS:
            _BEDS.pop(key).wk.close()
        _BEDS[key] = Bed(shape, kvd, n_slots)
    b = _BEDS[key]
    if armed:
        b.arm()
    b.restore()
    return b


@pytest.fixture(scope="module", autouse=True)
def _close_beds():
    yield
    for b in _BEDS.values():
        b.wk.close()
    _BEDS.clear()


def mixed_rows(n, stops=None):
    """row r by r % 4: a top_p row, a plain greedy row, a min_p row with penalties and a -inf bias, a processed greedy row; pool lengths
    differ, so the step's one k is the largest and the other rows draw from a clamped pool"""
    rows = []
    for r in range(n):
        d = [dict(strategy=TOP_P, pool_size=50, rng_state=W.rng_state_of_seed(100 + r)), dict(),
             dict(strategy=MIN_P, pool_size=20, rng_state=W.rng_state_of_seed(200 + r), state_slot=r),
             dict(strategy=GREEDY, pool_size=1, state_slot=r, rng_state=5)][r % 4]
        d["stop_ids"] = list((stops or {}).get(r, ()))
        rows.append(d)
    return rows


def _pooled(d):
    return d.get("strategy", GREEDY)[0] != 2 or d.get("state_slot", -1) >= 0


def loop_ref(b, n, rows, steps=STEPS):
    """`steps` one-step calls of the existing entry points with the feed rule on the host"""
    import torch
    wk = b.wk
    tok, pos, slots = b.t0[:n].copy(), b.pos[:n].copy(), np.arange(n, dtype=np.int32)
    rows = rows or [dict() for _ in range(n)]
    sel = [r for r in range(n) if _pooled(rows[r])]
    k = max([rows[r].get("pool_size", 1) for r in sel] + [1])
    live, emitted = [1] * n, [0] * n
    final = [int(d.get("rng_state", 0)) for d in rows]
    out = np.full((steps, n), -1, np.int32)
    if sel:
        params = W.sample_params_array([rows[r].get("strategy", GREEDY) for r in sel])
        params_dev = torch.from_numpy(params.view(np.uint8).copy()).cuda()
        states = torch.tensor([int(rows[r].get("rng_state", 0)) for r in sel], dtype=torch.int64).cuda()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in range(steps):
        if sel:
            wk.pool_adjust([rows[r].get("state_slot", -1) for r in sel])
            nxt, pools = wk.decode_batch_pool(tok, pos, slots, k, sel)
            counts, ids, vals = np.zeros(len(sel), np.int32), np.zeros((len(sel), k), np.int32), np.zeros((len(sel), k), np.uint16)
            for j, (pid, bits) in enumerate(pools):
                counts[j] = min(len(pid), rows[sel[j]].get("pool_size", 1))
                ids[j, :len(pid)] = pid
                vals[j, :len(pid)] = bits
            drawn, _ = W.sample_pool_rows(torch.from_numpy(counts).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(vals.view(np.int16)).cuda(),
                                          params_dev, states, err)
            torch.cuda.synchronize()
            drawn, st_now = drawn.cpu().numpy(), states.cpu().numpy()
        else:
            nxt = wk.decode_batch(tok, pos, slots)
        pairs = []
        for r in range(n):
            if not live[r]:
                continue
            t = int(drawn[sel.index(r)]) if r in sel else int(nxt[r])
            assert t >= 0
            out[s, r] = t
            emitted[r] += 1
            if r in sel:
                final[r] = int(st_now[sel.index(r)])
            if rows[r].get("state_slot", -1) >= 0:
                pairs.append((rows[r]["state_slot"], t))
            if t in rows[r].get("stop_ids", ()):
                live[r] = 0
            else:
                tok[r], pos[r] = t, pos[r] + 1
        if pairs:
            wk.logit_state_add([p[0] for p in pairs], [p[1] for p in pairs])
    wk.sync()
    return dict(out=out, emitted=emitted, rng=final, state=b.state(), kv=b.kv(n))


def fed(b, n, rows, steps=STEPS):
    out, emitted, states, _ = b.wk.decode_batch_steps(b.t0[:n], b.pos[:n], np.arange(n, dtype=np.int32), steps, rows)
    if rows is None:
        states = [0] * n
    return dict(out=out, emitted=[int(e) for e in emitted], rng=states, state=b.state(), kv=b.kv(n))


def assert_equal_runs(got, want, where):
    assert np.array_equal(got["out"], want["out"]), (where, got["out"], want["out"])
    assert got["emitted"] == want["emitted"] and got["rng"] == want["rng"], (where, got["emitted"], want["emitted"], got["rng"], want["rng"])
    assert (got["state"] is None) == (want["state"] is None) and (got["state"] is None or np.array_equal(got["state"], want["state"])), (where, "logit state")
    for sl, (a, w) in enumerate(zip(got["kv"], want["kv"])):
        for i, (x, y) in enumerate(zip(a, w)):
            assert np.array_equal(x, y), (where, "cache of slot %d, layer %d, %s" % (sl, i // 2, "kv"[i % 2]))


KVD = [dt.F16, dt.Q8_B32T2]
KVD_IDS = ["f16", "q8"]


@pytest.mark.parametrize("kvd", KVD, ids=KVD_IDS)
@pytest.mark.parametrize("n", [2, 8, 9, 16, 17])
def test_mixed_batch_equals_the_one_step_loop(kvd, n):
    """8 | 9: where the norm of the fused step becomes a launch of its own; 17: the first row count of the operand-order copies only"""
    b = _bed("test_gqa", kvd, 17)
    rows = mixed_rows(n)
    if not _one_fused_step(n):
        with pytest.raises(ia.IfaError) as e:
            fed(b, n, rows)
        assert e.value.code == -4
        return
    got = fed(b, n, rows)
    b.restore()
    want = loop_ref(b, n, rows)
    assert_equal_runs(got, want, "n = %d" % n)
    assert got["emitted"] == [STEPS] * n and (got["out"] >= 0).all()
    drawn = got["out"][:, 0::2]                     # the top_p and min_p rows: really drawn, not one id over and over
    assert len(set(int(t) for t in drawn.reshape(-1))) > 3, drawn
    for r in range(n):                              # the banned id never on a row with the -inf bias
        assert r % 4 < 2 or 400 not in got["out"][:, r]


@pytest.mark.parametrize("n", [2, 5])
def test_all_greedy_rows_equal_decode_batch(n):
    b = _bed("test_mha", dt.F16, 5, armed=False)
    got = fed(b, n, None)
    b.restore()
    want = loop_ref(b, n, None)
    assert_equal_runs(got, want, "greedy n = %d" % n)


def test_stops_freeze_a_row_and_nothing_else():
    n = 6
    b = _bed("test_gqa", dt.F16, 17)
    free = fed(b, n, mixed_rows(n))
    o = free["out"]
    # a token a row emits at step 2 and not before; a row whose first token stops it
    mid = next(r for r in range(n) if o[2, r] not in (o[0, r], o[1, r]))
    first = next(r for r in range(n) if r != mid)
    stops = {mid: [3, int(o[2, mid])], first: [int(o[0, first])]}
    b.restore()
    got = fed(b, n, mixed_rows(n, stops))
    assert got["emitted"][mid] == 3 and got["emitted"][first] == 1
    assert [int(t) for t in got["out"][:, mid]] == [int(t) for t in o[:3, mid]] + [-1] * (STEPS - 3)
    assert [int(t) for t in got["out"][:, first]] == [int(o[0, first])] + [-1] * (STEPS - 1)
    for r in range(n):                              # rows are independent given n
        if r not in stops:
            assert np.array_equal(got["out"][:, r], o[:, r]) and got["rng"][r] == free["rng"][r]
    # the frozen row's cache: the rows of the unstopped run up to its position, untouched behind it
    for r, kept in ((mid, 3), (first, 1)):
        for i, (a, w, snap) in enumerate(zip(got["kv"][r], free["kv"][r], b.snap[r])):
            row = a.size // MAX_CTX
            cut = (int(b.pos[r]) + kept) * row
            assert np.array_equal(a[:cut], w[:cut]) and np.array_equal(a[cut:], snap[cut:]), (r, i)
    b.restore()
    assert_equal_runs(got, loop_ref(b, n, mixed_rows(n, stops)), "stops")


def test_all_rows_stopped_before_the_last_step():
    n = 5
    b = _bed("test_gqa", dt.Q8_B32T2, 17)
    o = fed(b, n, mixed_rows(n))["out"]
    stops = {}
    for r in range(n):
        at = next(s for s in range(STEPS - 1) if s >= min(r, 3) and o[s, r] not in o[:s, r])
        stops[r] = [int(o[at, r])]
    b.restore()
    got = fed(b, n, mixed_rows(n, stops))
    assert (got["out"][STEPS - 1] == -1).all() and max(got["emitted"]) < STEPS and min(got["emitted"]) >= 1
    b.restore()
    assert_equal_runs(got, loop_ref(b, n, mixed_rows(n, stops)), "all stopped")


def test_the_other_steps_are_not_disturbed():
    n = 4
    b = _bed("test_gqa", dt.F16, 17)
    wk = b.wk
    slots = np.arange(n, dtype=np.int32)
    p = _capi.SampleParams(4, 0.9, 0.9, 8, 0.05, 50)

    def others():
        b.restore()
        batch = wk.decode_batch(b.t0[:n], b.pos[:n], slots)
        greedy, _ = wk.decode(int(b.t0[0]), int(b.pos[0]), 4)
        b.restore()
        sampled, st, _ = wk.decode_sampled(int(b.t0[0]), int(b.pos[0]), 4, p, W.rng_state_of_seed(5))
        b.restore()
        draft = wk.decode_draft([int(b.t0[0]), 5, 6], int(b.pos[0]))
        return [int(t) for t in batch], [int(t) for t in greedy], [int(t) for t in sampled], st, [int(t) for t in draft]

    before = others()
    b.restore()
    first = fed(b, n, mixed_rows(n))
    b.restore()
    again = fed(b, n, mixed_rows(n))                 # the replayed steps give the captured ones' result
    assert_equal_runs(again, first, "replay")
    assert others() == before


def _refused(b, code, word, n=3, steps=STEPS, rows="mixed", tokens=None, pos=None, slots=None):
    L = ia.lib()
    rows = mixed_rows(n) if rows == "mixed" else rows
    with pytest.raises(ia.IfaError) as e:
        b.wk.decode_batch_steps(b.t0[:n] if tokens is None else tokens, b.pos[:n] if pos is None else pos,
                                np.arange(n, dtype=np.int32) if slots is None else slots, steps, rows)
    assert e.value.code == code and word in str(e.value) and "ifa_model_decode_batch_steps" in str(e.value), (code, word, str(e.value))


def test_refusals_touch_nothing():
    b = _bed("test_gqa", dt.F16, 17)
    kv0, st0 = b.kv(3), b.state()
    for steps in (0, 257):
        _refused(b, -1, "n_steps", steps=steps)
    _refused(b, -1, "outside max_ctx", pos=np.array([1, 5, MAX_CTX - STEPS + 1], np.int32))
    _refused(b, -1, "outside max_ctx", pos=np.array([1, -1, 3], np.int32))
    _refused(b, -1, "used twice", slots=np.array([0, 1, 0], np.int32))
    _refused(b, -1, "KV slot 17", slots=np.array([0, 1, 17], np.int32))
    _refused(b, -1, "outside the vocabulary", tokens=np.array([1, 2, b.V], np.int32))
    for patch, word in ((dict(strategy=(10, 1.0, 1.0, 1, 0.0)), "strategy 10"), (dict(pool_size=0), "pool_size 0"), (dict(pool_size=257), "pool_size 257"),
                        (dict(stop_ids=list(range(9))), "n_stop 9"), (dict(state_slot=17), "state slot 17 has no logit state"), (dict(state_slot=-2), "state slot -2")):
        rows = mixed_rows(3)
        rows[0].update(patch)
        _refused(b, -1, word, rows=rows)
    # not ONE fused, captured step
    _refused(b, -4, "one row", n=1)
    _refused(b, -4, "run as steps of", n=33, tokens=np.ones(33, np.int32), pos=np.ones(33, np.int32), slots=np.arange(33, dtype=np.int32), rows=None)
    for name, value, word in (("exact_order", 1, "exact_order"), ("perf_stat", 1, "perf_stat"), ("graph", 0, "not captured"), ("batch_fused", 0, "op by op")):
        b.wk.set_option(name, value)
        try:
            _refused(b, -4, word)
        finally:
            b.wk.set_option(name, 1 - value)
    for a, w in zip(b.kv(3), kv0):
        for x, y in zip(a, w):
            assert np.array_equal(x, y)
    assert np.array_equal(b.state(), st0)
    # a row without a candidate: every id excluded leaves the drawn rows empty pools
    b.wk.set_pool_excluded(list(range(b.V)))
    try:
        _refused(b, -4, "step 0, row 0 had no token to draw")
    finally:
        b.wk.set_pool_excluded([])
    b.restore()
    assert fed(b, 3, mixed_rows(3))["emitted"] == [STEPS] * 3


def test_a_worker_without_logit_state_refuses_a_state_slot():
    b = _bed("test_mha", dt.F16, 5, armed=False)
    rows = mixed_rows(3)
    _refused(b, -1, "has no logit state", rows=rows)


def test_moe_rows_routed_on_the_device():
    n = 3
    assert _one_fused_step(n, has_moe=1)
    b = _bed("test_moe", dt.F16, 3)
    rows = mixed_rows(n)
    got = fed(b, n, rows)
    b.restore()
    assert_equal_runs(got, loop_ref(b, n, rows), "moe")
