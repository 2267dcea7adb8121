"""-m gpu: the batched, draft and device-fed steps of a 256-wide model at level 2 of ifa_attention_mfma_heads: k_dec_attn256_batch
(csrc/ifa_decode_attn256.h) and k_draft_kv_store at 256.  What (a), (b) and (c) hold, the models and the figures: docs/decode_batch_heads256.md.
ifa_model_batch_steps_rows > 0 says that the batched step is the fused, captured one; without the kernel it is 0 and every test here fails."""
import numpy as np
import pytest
import torch

import inferflow_amd as ia
from inferflow_amd.engine import EngineError, InferenceEngine
from tests import decode_attn_util as U
from tests import engine_fixtures as fx
from tests import gpu_util as g
from tests.test_gpu_attn_heads16 import _Switch
from tests.test_gpu_decode_attn_edges import F16, KV_ID, Q8, TOK, _report
from tests.test_gpu_decode_attn_heads256 import SHAPES, _build
from tests.test_gpu_generate_batch_engine import PROMPTS, _equal_run
from tests.test_gpu_prompt_routes import _agree

pytestmark = pytest.mark.gpu

# keys per row of one step: the quad and first-pass edges, one 64-key pass, the P.V groups of 64 keys, several passes
MIXES = [(1, 2, 64, 65), (3, 5, 63, 257), (4, 128, 256, 513), (127, 129), (255, 1)]
KERNEL = [(sh, kvd, {}, MIXES) for sh in SHAPES for kvd in (F16, Q8)] + [
    ("2over1", F16, dict(use_alibi=1), [(64, 65, 257, 1)]), ("4over4", Q8, dict(partial_rotary=0.5), [(65, 2)])]
OP_BY_OP = "the batched step of this model runs op by op"


def _fused_rows(wk):
    return ia.lib().ifa_model_batch_steps_rows(wk._h)


@pytest.mark.parametrize("shape,kvd,geo_kw,mixes", KERNEL, ids=["%s-%s%s" % (s, KV_ID[k], "".join("-" + x for x in kw)) for s, k, kw, _ in KERNEL])
def test_batched_kernel_against_float64(shape, kvd, geo_kw, mixes):
    with _Switch(2):
        wk, _, geo = _build(shape, kvd, 640, **geo_kw)
        assert _fused_rows(wk) == 32
        wk.kv_slots(4)
        rb, width, stats, row_fig = geo.row_bytes, geo.qd + 2 * geo.kv_dim, [], [0, 0]
        for ctxs in mixes:
            n = len(ctxs)
            toks, pos, slots = [TOK + r for r in range(n)], [c - 1 for c in ctxs], list(range(n))
            wk.decode_batch(toks, pos, slots)
            bqkv = wk.read_buffer("rows_bqkv").view(np.float16).reshape(32, width)[:n].copy()
            cases = [list(U.make_cases(bqkv[r], pos[r], geo)) for r in range(n)]
            for i in range(max(len(cs) for cs in cases)):           # (a row with fewer cases goes round again)
                cur = [cs[i % len(cs)] for cs in cases]
                for r, c in enumerate(cur):
                    wk.select_kv(r)
                    for name, rows in (("kcache", c.k_rows), ("vcache", c.v_rows)):
                        if pos[r]:
                            wk.write_buffer(name, rows[:pos[r]])
                wk.decode_batch(toks, pos, slots)
                att = wk.read_buffer("rows_att", nbytes=n * geo.qd * 2).view(np.float16).reshape(n, geo.qd)
                assert np.array_equal(wk.read_buffer("rows_bqkv").view(np.float16).reshape(32, width)[:n], bqkv), ("rows_bqkv changed", ctxs)
                for r, c in enumerate(cur):
                    p, where = pos[r], (ctxs, r, c.family, c.needle)
                    wk.select_kv(r)
                    kc, vc = (wk.read_buffer(name, nbytes=ctxs[r] * rb).reshape(ctxs[r], rb) for name in ("kcache", "vcache"))
                    assert np.array_equal(kc[:p], c.k_rows[:p]) and np.array_equal(vc[:p], c.v_rows[:p]), ("a cached row changed", where)
                    fig = U.check_new_row(kc[p], vc[p], bqkv[r], p, geo)
                    row_fig = [row_fig[0] + fig[0] * (i == 0), row_fig[1] + fig[1] * (i == 0)]
                    stats.append((U.check_att(att[r], c), c.family, c.n, c.needle))
        _report("batch 256 %s %s%s" % (shape, KV_ID[kvd], "".join(" " + x for x in geo_kw)), stats)
        print("row p: %d of %d values / codes differ from the reference's" % (row_fig[1], row_fig[0]))
        wk.close()


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
def test_draft_rows_are_bit_identical_to_independent_queries(kvd):
    """tests/test_gpu_decode_draft.py's assertion at 256, across the 64- and 256-key edges"""
    with _Switch(2):
        wk, s, geo = _build("2over1", kvd, 640, layers=2)
        assert _fused_rows(wk) == 32
        V, rb = s["vocab"], geo.row_bytes
        wk.kv_slots(8)
        rng = np.random.default_rng(41)
        prompt, drafts = rng.integers(3, V, 252).astype(np.int32), rng.integers(3, V, 7).astype(np.int32)
        for n, pos0 in ((8, 1), (8, 60), (8, 252), (2, 63)):
            wk.select_kv(0)
            toks = np.concatenate([[int(wk.forward(prompt[:pos0], 0))], drafts[:n - 1]]).astype(np.int32)
            lgd, lgb = (torch.empty((n, V), dtype=torch.float16, device="cuda") for _ in range(2))
            ids_d = wk.decode_draft(toks, pos0, lgd)
            mine = [(wk.read_buffer("kcache", l).copy(), wk.read_buffer("vcache", l).copy()) for l in range(2)]
            for i in range(1, n):
                wk.kv_copy(0, i, pos0 + n)
            wk.sync()
            ids_b = wk.decode_batch(toks, [pos0 + i for i in range(n)], list(range(n)), lgb)
            assert ids_d.tolist() == ids_b.tolist(), (n, pos0)
            assert np.array_equal(g.host(lgd).view(np.uint16), g.host(lgb).view(np.uint16)), (n, pos0)
            for i in range(n):
                wk.select_kv(i)
                a, b = (pos0 + i) * rb, (pos0 + i + 1) * rb
                for l in range(2):
                    for kv, name in enumerate(("kcache", "vcache")):
                        assert np.array_equal(wk.read_buffer(name, l)[a:b], mine[l][kv][a:b]), (n, pos0, i, l, name)
        wk.close()


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
def test_model_runs_batched_steps_and_short_prompts_fused_at_level_2(kvd):
    wk, s, _ = _build("2over1", kvd, 320, layers=2)
    V, N = s["vocab"], 17
    prompt = (np.arange(250, dtype=np.int32) * 7 + 3) % V
    toks, pos, slots = list(range(5, 5 + N)), [9 + r % 3 for r in range(N)], list(range(N))
    wk.kv_slots(N)

    def prefill():                              # (the prompts op by op both times: only the batched step sees the level)
        with _Switch(0):
            for r in range(N):
                wk.select_kv(r)
                wk.forward(prompt[r:r + pos[r]], 0)

    def step(n):
        lg = torch.empty((n, V), dtype=torch.float16, device="cuda")
        return wk.decode_batch(toks[:n], pos[:n], slots[:n], lg).tolist(), g.host(lg).astype(np.float32), g.host(lg).view(np.uint16).copy()

    # 2, 9 and 17 rows: fused norm, separate norm, MO rows
    runs = {}
    for lvl in (0, 2):
        prefill()
        with _Switch(lvl):
            assert _fused_rows(wk) == (32 if lvl == 2 else 0)
            runs[lvl] = [step(n) for n in (2, 9, 17)]
    for (t2, l2, _), (t0, l0, _) in zip(runs[2], runs[0]):
        assert t2 == t0
        for r in range(len(t2)):
            ok, why = _agree(l2[r], l0[r])
            assert ok, (len(t2), r, why)
    # a 20-token prompt
    rows = {}
    for lvl in (0, 2):
        with _Switch(lvl):
            wk.select_kv(0)
            lg = torch.empty((20, V), dtype=torch.float16, device="cuda")
            tok = int(wk.forward(prompt[:20], 0, lg))
            rows[lvl] = (tok, wk.prompt_route()["kind"], g.host(lg).astype(np.float32))
    assert rows[0][1] != "rows" and rows[2][1] == "rows" and rows[0][0] == rows[2][0], (rows[0][:2], rows[2][:2])
    for r in range(20):
        ok, why = _agree(rows[2][2][r], rows[0][2][r])
        assert ok, (r, why)
    # the device-fed steps: refused below level 2 with the text they always gave, accepted at 2 with decode_batch's tokens
    prefill()
    for lvl in (0, 1):
        with _Switch(lvl), pytest.raises(ia.IfaError, match=OP_BY_OP):
            wk.decode_batch_steps(toks[:2], pos[:2], slots[:2], 2)
    with _Switch(2):
        fed = wk.decode_batch_steps(toks[:2], pos[:2], slots[:2], 2)[0]
        assert fed[0].tolist() == runs[2][0][0]
        assert wk.decode_batch(fed[0], [p + 1 for p in pos[:2]], slots[:2]).tolist() == fed[1].tolist()
    # captured steps do not outlive the level they were captured under: 2 -> 0 -> 2 on one worker, the step replayed each time
    prefill()
    wk.set_option("batch_graph", 1)
    for lvl in (2, 0, 2):
        with _Switch(lvl):
            first, again = step(2), step(2)
            assert np.array_equal(first[2], again[2]) and np.array_equal(first[2], runs[lvl][0][2]), ("captured under another level", lvl)
    wk.close()


def test_engine_key_level_2_and_generate_batch(tmp_path):
    """.ini level 2: GenerateBatch runs device-fed rounds with the loop's tokens; `true`: refused (model_info "batch_generate" does not ask the model)"""
    s = dict(fx.SHAPE, **SHAPES["2over1"])

    def engine(name, level):
        ini, _ = fx.write_model_dir(str(tmp_path / name), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", ctx=64, s=s)
        keys = "attention_mfma_heads = %s\ndevice_sampling_pool = true\nbatch_generate_round_steps = 4\n" % level
        text = open(ini).read().replace("return_output_tensors = false", "return_output_tensors = false\n" + keys)
        open(ini, "w").write(text)
        return InferenceEngine.from_ini(ini)

    with _Switch(0):                            # (Init sets the process-wide switch from the key: put back on the way out)
        one = engine("one", "true")
        assert g.capi().ifa_attention_mfma_heads(-1) == 1
        ids = [one.add_query(p) for p in PROMPTS[:2]]
        with pytest.raises(EngineError, match="fused batched step"):
            one.generate_batch([(q, 6) for q in ids])
        one.close()
        gen, loop = engine("gen", "2"), engine("loop", "2")
        assert g.capi().ifa_attention_mfma_heads(-1) == 2 and gen.model_info("batch_generate") == 1
        _equal_run(gen, loop, [(p, {}) for p in PROMPTS[:2]], [10, 7])
        assert gen.model_info("batch_generate_rounds") >= 2 and loop.model_info("batch_generate_rounds") == 0
        gen.close()
        loop.close()
