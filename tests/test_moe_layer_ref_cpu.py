"""No GPU: the host half of the MoE layer suite (tests/moe_layer_util.py).  For every routing tests/test_gpu_moe_layer_edges.py runs: the design
margins, the plan the case is designed for against the pure plan (ifa_moe_plan), and -- on host-made inputs of the case's own lists and shapes --
that every fault of docs/moe_layer_edges.md moves at least one element by SENSITIVITY x its bound and is rejected by the assertion the device
test calls, while the oracle's own output passes."""
import numpy as np
import pytest

from inferflow_amd import worker as W
from tests import moe_layer_util as U

CASES = U.all_cases()
_EXPERTS = {}


def _experts(E, ffn):
    if (E, ffn) not in _EXPERTS:
        _EXPERTS[(E, ffn)] = U.host_experts(E, ffn)
    return _EXPERTS[(E, ffn)]


def test_case_list():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    b = [c for c in CASES if c.mode == "batch"]
    assert {c.n for c in b} == {2, 4, 8, 9, 16, 32} and {c.n for c in CASES if c.mode == "prompt"} == {2, 8, 9, 17, 33, 65, 129, 193}
    assert {c.ffn for c in CASES} == {512, 4352}
    # the counts the routings are named for
    by = {c.id: c for c in CASES}
    assert by["batch-E8-n8-f512-groups"].counts().tolist() == [1, 5, 1, 3, 2, 4, 0, 0]
    assert by["batch-E8-n4-f512-spread"].counts().tolist() == [1] * 8 and by["batch-E8-n8-f512-spread"].counts().tolist() == [1] * 8
    assert by["batch-E8-n8-f512-drop"].counts().sum() == 12 and by["batch-E8-n8-f512-ends"].counts().tolist() == [8, 0, 0, 0, 0, 0, 0, 8]
    assert by["batch-E8-n9-f512-tile9-small8-single"].counts().tolist()[:3] == [9, 8, 1] and by["batch-E8-n32-f512-even"].counts().tolist() == [8] * 8
    for T, tiles in ((65, [64, 1]), (129, [64, 64, 1])):
        c = by["prompt-E8-n%d-f512-first0" % T]
        assert c.counts()[0] == T and c.counts()[7] == 1 and c.counts()[6] == 2
    c = by["prompt-E4-n193-f512-first0"]
    assert c.counts().tolist() == [193, 190, 2, 1]
    # rows 0 of the groups: a group of 2, 3, 4, 5 and 8 rows starts at an odd entry somewhere
    odd = set()
    for c in b:
        r, _ = None, None
        L = U.M.build_lists(c.sel(), np.zeros(c.sel().shape, np.float16), c.n, c.K, c.E, 64, 8)
        odd |= {int(s[2]) for s in L.smalls if s[1] % 2}
    assert {2, 3, 4, 5, 8} <= odd, odd


@pytest.mark.parametrize("rc", CASES, ids=[c.id for c in CASES])
def test_design_margins(rc):
    gap, kept, dropped, wdiff = U.check_margins(rc)
    print("moe-layer-margins %-40s logit gap %.2f  kept p >= %.2e  dropped p <= %.1e  weight difference %.3f" % (rc.id, gap, kept, dropped, wdiff))


@pytest.mark.parametrize("rc", CASES, ids=[c.id for c in CASES])
def test_plan_of_the_case(rc):
    sets = U.OPTION_SETS if rc.mode == "batch" and rc.n <= 8 else U.OPTION_SETS[:1]
    for name, opts in sets:
        for have_mo in (1, 0):
            p = W.moe_plan(**U.plan_facts(rc, opts, have_mo))
            want = U.expected_plan(rc, opts, have_mo)
            assert {k: p[k] for k in U.PLAN_KEYS} == want, (name, have_mo, p)
    d = U.expected_plan(rc)
    if rc.name == "router":
        assert d["router"] == "fused"
    elif rc.mode == "batch":
        assert (d["kind"], d["router"]) == ("device_singles" if rc.n <= 8 else "device_grouped", "fused")
        assert d["side_stream"] == int(rc.n <= 8)
    else:
        assert d["router"] == "ops" and d["tile_rows"] == (128 if rc.n == 193 else 64) and d["small_max"] == (8 if rc.n <= 32 else 0)


HOST_FAULT_CASES = [c for c in CASES if c.n <= 65 and c.name != "router"]      # (the router cases add no list shape; 129 and 193 rows: the 65-row lists with more tiles)


@pytest.mark.parametrize("rc", HOST_FAULT_CASES, ids=[c.id for c in HOST_FAULT_CASES])
def test_faults_move_and_are_rejected(rc):
    ref, r = U.host_step(rc, _experts(rc.E, rc.ffn))
    L = ref.launches()
    for name, lr in L.items():
        U.check_launch(U.device_like(lr), lr)                 # the oracle's own rows pass
    worst = {}
    for name, launch, f64 in ref.faults():
        lr = L[launch]
        ratio = float((np.abs(f64 - lr.f64) / lr.bound).max())
        assert ratio >= U.SENSITIVITY, (rc.id, name, launch, ratio)
        with pytest.raises(AssertionError):
            U.check_launch(U.device_like(lr, f64), lr)
        worst[name] = min(worst.get(name, np.inf), ratio)
    assert worst
    print("moe-layer-faults %-40s %d faults, smallest margin %.1f x bound (%s)" % (rc.id, len(worst), min(worst.values()), min(worst, key=worst.get)))


def test_every_fault_kind_is_shown_by_the_cases():
    seen = set()
    for rc in HOST_FAULT_CASES:
        if rc.ffn != 512 or rc.n > 16:
            continue
        ref, _ = U.host_step(rc, _experts(rc.E, rc.ffn))
        seen |= {next(k for k in U.FAULT_KINDS if k in name) for name, _, _ in ref.faults()}
    assert seen == set(U.FAULT_KINDS), set(U.FAULT_KINDS) - seen
