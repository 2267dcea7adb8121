"""-m gpu: the worker's memory (csrc/ifa_buf.h owners over two counted spaces) on the device.
  * a worker's whole life -- prompt, decode, slots, batched steps, pools with logit processors, scoring, slot copy, draft step,
    close -- leaves no block behind (ifa_debug_live_allocs);
  * an allocation that fails while a step grows its buffers (ifa_debug_alloc_fail_at, walked over EVERY allocation of the step)
    fails the call with nothing leaked and leaves the worker as it was: the step that finally fits answers like an untouched
    twin, and the single-query step captured before still replays;
  * the same for ifa_model_kv_slots."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd import dtypes as dt, synth
from tests import gpu_util as g
from tests.test_gpu_waits import _close, _prefill_slots

pytestmark = pytest.mark.gpu


def _build(preset):
    return synth.build(preset, dt.Q4_B32T1A, dt.F16, max_ctx=48, quant_threshold=0, std=0.06)


def _live():
    n, b = C.c_longlong(-1), C.c_longlong(-1)
    ia.check(g.capi().ifa_debug_live_allocs(C.byref(n), C.byref(b)))
    return n.value, b.value


def _fail_at(k):
    ia.check(g.capi().ifa_debug_alloc_fail_at(k))


def _life_cycle(preset):
    wk, _, s = _build(preset)
    V = s["vocab"]
    rng = np.random.default_rng(5)
    alive = _live()
    prompt = rng.integers(3, V, 5).astype(np.int32)
    nxt = wk.forward(prompt, 0)
    toks, _ = wk.decode(nxt, 5, 3)
    wk.kv_slots(12)
    cur = [int(toks[-1])] + [int(t) for t in rng.integers(3, V, 11)]
    pos = [8] + [0] * 11
    lg = torch.empty((12, V), dtype=torch.float16, device="cuda")
    out = wk.decode_batch(cur, pos, list(range(12)), lg)
    wk.logit_state_reset(0, prompt, rep=1.2, freq=0.1, pres=0.1, bias={5: -1.0})
    wk.logit_state_reset(1, [], rep=1.1)
    wk.pool_adjust([0, 1])
    out2, pools, lse = wk.decode_batch_pool_lse([int(t) for t in out], [p + 1 for p in pos], list(range(12)), 8, [0, 1])
    assert len(pools) == 2 and len(lse) == 2 and np.isfinite(lse).all()
    wk.select_kv(2)
    score_toks = rng.integers(3, V, 6).astype(np.int32)
    _, lse_rows, _ = wk.forward_score(score_toks, 0, np.roll(score_toks, -1))
    assert np.isfinite(lse_rows).all()
    wk.kv_copy(2, 3, 6)
    draft = wk.decode_draft([int(t) for t in rng.integers(3, V, 4)], 6)
    assert len(draft) == 4
    during = _live()
    wk.close()
    return alive, during


@pytest.mark.parametrize("preset", ["test_mha", "test_moe"])
def test_a_worker_life_cycle_leaves_no_allocation_behind(preset):
    gc.collect()
    before = _live()
    after = []
    for cycle in range(3):
        alive, during = _life_cycle(preset)
        assert alive[0] > before[0] and during[0] > alive[0], (before, alive, during)      # a live worker is counted
        after.append(_live())
        print(preset, "cycle", cycle, "before", before, "alive", alive, "during", during, "after", after[-1])
    assert after[1] == after[0] and after[2] == after[0], (before, after)
    assert after[0] == before, (before, after)      # (the process-level caches do not go through the counted spaces)


def test_failed_growth_of_a_batched_step_leaves_the_worker_usable():
    n = 12
    wk, _, s = _build("test_mha")
    ref, _, _ = _build("test_mha")
    V = s["vocab"]
    try:
        for w in (wk, ref):
            w.kv_slots(n)
        cur, pos = _prefill_slots(ref, V, n, 11)
        cur2, pos2 = _prefill_slots(wk, V, n, 11)
        assert cur2 == cur and pos2 == pos
        for w in (wk, ref):
            w.select_kv(0)
        first_wk, _ = wk.decode(cur[0], pos[0], 1)             # captures the single-query step
        first_ref, _ = ref.decode(cur[0], pos[0], 1)
        assert int(first_wk[0]) == int(first_ref[0])
        lg_a = torch.empty((n, V), dtype=torch.float16, device="cuda")
        lg_b = torch.empty((n, V), dtype=torch.float16, device="cuda")
        ta, k_ok = None, 0
        for k in range(1, 65):
            live = _live()
            _fail_at(k)
            try:
                ta = wk.decode_batch(cur, pos, list(range(n)), lg_a)
            except ia.IfaError as e:
                # anything but the injected failure ends the test here (nothing further runs on the device: finally only disarms)
                assert "simulated" in str(e), (k, str(e))
                assert _live()[0] == live[0], (k, live, _live())
                continue
            k_ok = k
            break
        _fail_at(0)
        print("the step's allocations:", k_ok - 1)
        assert ta is not None and k_ok > 1, k_ok
        tb = ref.decode_batch(cur, pos, list(range(n)), lg_b)
        ok, why = _close(g.host(lg_a), g.host(lg_b))
        assert ok, why
        gaps = np.sort(g.host(lg_b).astype(np.float32), axis=1)
        for i in range(n):
            if gaps[i, -1] - gaps[i, -2] > 0.05:
                assert int(ta[i]) == int(tb[i]), i
        # the single-query step again, same token at the same position (it rewrites the same cache row)
        again_wk, _ = wk.decode(cur[0], pos[0], 1)
        again_ref, _ = ref.decode(cur[0], pos[0], 1)
        assert int(again_wk[0]) == int(again_ref[0]) == int(first_ref[0])
    finally:
        g.capi().ifa_debug_alloc_fail_at(0)
    wk.close(); ref.close()


def test_failed_kv_slots_growth_keeps_the_slots_it_had():
    wk, _, s = _build("test_mha")
    try:
        one_slot = _live()
        for k in (1, 2 * s["layers"]):
            _fail_at(k)
            with pytest.raises(ia.IfaError, match="simulated"):
                wk.kv_slots(3)
            assert _live() == one_slot, (k, one_slot, _live())
        _fail_at(0)
        wk.kv_slots(3)
        three = _live()
        assert three[0] == one_slot[0] + 2 * 2 * s["layers"], (one_slot, three)
        cur, pos = _prefill_slots(wk, s["vocab"], 3, 7)
        assert len(wk.decode_batch(cur, pos, [0, 1, 2])) == 3
    finally:
        g.capi().ifa_debug_alloc_fail_at(0)
    wk.close()
