"""-m gpu: prompt attention for head_dim 256 on the matrix cores (k_attention_heads16<256, Q8> behind csrc/ifa_attn_heads256_plan.h), through
ifa_attention with ifa_attention_mfma_heads(1), against the oracle's arithmetic and plain float64 math at its wave (16 queries), tile
(64 queries) and key-block (32 keys) edges, and at those of the 128-query design it was measured against (32, 128).  Shapes: tests/test_attn_heads256_plan_cpu.py; inputs (dense / flat / needle), references
and both bounds: tests/prompt_attn_util.py, unchanged from docs/prompt_attention_edges.md; the launch itself (sentinel rows around out, two
bit-identical launches, q / K / V unchanged, nothing started after a device error): tests/test_gpu_prompt_attn_edges.py.  With the switch
at 0 the same input through k_attention lies within that document's cross-kernel figure, 4e-3 (x max(1, max|V|) on flat and needle).
Then two layers of a 256-wide model through the worker, switch on against switch off.  Figures: docs/prompt_attention_heads256.md."""
import numpy as np
import pytest

from inferflow_amd import dtypes as dt, synth
from tests import prompt_attn_util as U
from tests import test_gpu_prompt_attn_edges as E
from tests import test_gpu_prompt_routes as R
from tests.test_attn_heads256_plan_cpu import IDS, SHAPES, heads256_plan
from tests.test_gpu_attn_heads16 import _Switch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_heads256_against_float64_and_the_oracle(sh):
    failed, errs = [], []
    assert heads256_plan(sh.kvd, sh.n_ctx, sh.qt, sh.prefix, sh.heads, sh.kv_heads, sh.hd)["error"] == 0
    for case in U.make_cases(sh):
        with _Switch(1):
            out = E._launch(case)
        with _Switch(0):
            scalar = E._launch(case)
        try:
            errs.append(float(U.check_rows(out, case).max()))
        except AssertionError as e:
            failed.append(str(e))
        cross = 4e-3 * (1.0 if case.family == "dense" else max(1.0, case.vmax))
        d = float(np.abs(out.astype(np.float64) - scalar.astype(np.float64)).max())
        if d > cross:
            failed.append("against k_attention: %.3g > %.3g (%s)" % (d, cross, case.tag))
    errs.sort()
    print("attn-heads256 %-40s %4d cases  median %.3f  worst %.3f" % (sh.id, len(errs), errs[len(errs) // 2] if errs else 0, errs[-1] if errs else 0))
    assert not failed, "%d launches: %s" % (len(failed), " | ".join(failed[:12]))


def test_model_with_256_wide_heads_switch_on_against_off():
    """a 70-token prompt through two layers of dim 512 = 2 heads x 256 over 1 kv head: every logits row within the bound
    tests/test_gpu_prompt_routes.py applies between prompt routes, and the same greedy token"""
    wk, _, s = synth.build("test_gqa", dt.F16, dt.F16, max_ctx=96, dim=512, heads=2, kv_heads=1, head_dim=256)
    toks = np.random.default_rng(256).integers(3, s["vocab"], 70).astype(np.int32)
    out = {}
    for on in (0, 1):
        with _Switch(on):
            out[on] = R._rows(wk, toks, s["vocab"])
    wk.close()
    ok, why = R._agree(out[1][1], out[0][1])
    assert ok, why
    assert out[1][0] == out[0][0]
