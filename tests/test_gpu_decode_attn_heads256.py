"""-m gpu: the fused decode step of a 256-wide model (Gemma's head size) behind ifa_attention_mfma_heads(1): k_dec_attn256 (one
workgroup per head, a key row split over a quad of lanes) and k_dec_attn256_scores -> k_dec_attn_pv<256> -> k_dec_attn_combine<256>
(keys split over workgroups), csrc/ifa_decode_attn256.h, docs/decode_attention_heads256.md.

The walks, the inputs and every assertion are those of tests/test_gpu_decode_attn_edges.py and tests/decode_attn_util.py (one step at
position p over rows the test wrote: att against oracle.attention within 6e-3 x max(1, max|V|) and against float64 within
max(2 x d_ref, one F16 ulp at max|out|); cache row p; attq bit-equal to the reference quantiser of the device's own att; rows 0 .. p - 1
unchanged; the planned route at the first step of every context).  The walks use ONE layer, as that helper requires ("att" and "dqkv" are
the last layer's, the caches read are layer 0's); the engine-level cases below use two.  The quad adds a key's products in another
order than the reference's single chain, so the float64 bound is the one that matters here.

The contexts: 1 .. 5 (quad and first-pass edges), 63 / 64 / 65 (one 64-key pass), 127 .. 129, 255 .. 257 (P.V groups of 8 x 8 keys and
the prefetch tail), 513; split walks from 1 key (one workgroup: reach 1) over 7 .. 9, 31 .. 33, 63 .. 65 (fewer keys than splits, one
64-key chunk) to 257 and 700."""
import numpy as np
import pytest

from inferflow_amd import _capi, dtypes as dt, synth
from inferflow_amd import worker as W
from inferflow_amd.engine import InferenceEngine
from tests import decode_attn_util as U
from tests import engine_fixtures as fx
from tests.test_gpu_attn_heads16 import _Switch
from tests.test_gpu_decode_attn_edges import F16, KV_ID, Q8, _assert_route, _walk
from tests.test_gpu_prompt_routes import _agree

pytestmark = pytest.mark.gpu

N_ONE_WG = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
N_SPLIT = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257, 700)
SHAPES = {"2over1": dict(dim=512, heads=2, kv_heads=1, head_dim=256), "4over4": dict(dim=1024, heads=4, kv_heads=4, head_dim=256)}
ONE_WG = dict(kind="one_workgroup", pb=256, kt=0, ul=0, nsplits=0, chain=0)
OLD_REASON = "fused attention supports head_dim 32/48/64/80/96/128"


def _build(shape, kvd, max_ctx, layers=1, **geo_kw):
    s = SHAPES[shape]
    wk, _, spec = synth.build("test_gqa", dt.Q4_B32T1A, kvd, max_ctx=max_ctx, layers=layers, quant_threshold=0, std=0.06, **s, **geo_kw)
    return wk, spec, U.Geo(s["heads"], s["kv_heads"], 256, kvd, **geo_kw)


ONE = [(sh, kvd, {}, N_ONE_WG) for sh in SHAPES for kvd in (F16, Q8)] + [
    ("2over1", F16, dict(use_alibi=1), (64, 65, 257)), ("2over1", Q8, dict(use_alibi=1), (64, 65, 257)), ("4over4", F16, dict(partial_rotary=0.5), (65,))]


@pytest.mark.parametrize("shape,kvd,geo_kw,ns", ONE, ids=["%s-%s%s" % (s, KV_ID[k], "".join("-" + x for x in g)) for s, k, g, _ in ONE])
def test_one_workgroup_per_head(shape, kvd, geo_kw, ns):
    with _Switch(1):
        wk, _, geo = _build(shape, kvd, 640, **geo_kw)
        ok, why = wk.fused_supported()
        assert ok, why
        wk.set_option("attn_split_ctx", 0)
        _walk(wk, geo, ns, [], "one-wg 256 %s %s" % (shape, KV_ID[kvd]), lambda n: ONE_WG)
        wk.close()


@pytest.mark.parametrize("nsplits", [8, 32])
@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_keys_split_over_workgroups(shape, kvd, nsplits):
    with _Switch(1):
        wk, _, geo = _build(shape, kvd, 704)
        wk.set_option("attn_split_ctx", 1)
        wk.set_option("attn_nsplits", nsplits)
        _walk(wk, geo, N_SPLIT, [], "split 256 %s %s x%d" % (shape, KV_ID[kvd], nsplits),
              lambda n: ONE_WG if n == 1 else dict(kind="split", nsplits=nsplits, split=8, lds_scores=16, chain=0))
        wk.close()


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
def test_model_decodes_on_the_fused_step_with_the_switch_on(kvd):
    """two layers, 12 steps behind a 20-token prompt op by op (switch off: fused_supported false with the reason it always gave) and
    fused (switch on); then spans across 64 / 128 / 256 keys as one call and as one-step calls, bit for bit; then the batched step,
    which keeps its own kernels and must not notice the switch.  Fails without the 256-wide decode kernels: fused_supported stays false."""
    wk, s, _ = _build("2over1", kvd, 320, layers=2)
    V = s["vocab"]
    prompt = (np.arange(250, dtype=np.int32) * 7 + 3) % V
    runs = {}
    for on in (0, 1):
        with _Switch(on):
            ok, why = wk.fused_supported()
            assert ok == bool(on) and (on or why == OLD_REASON), (on, ok, why)
            wk.reset()
            t, toks, rows = int(wk.forward(prompt[:20], 0)), [], []
            for i in range(12):
                t = int(wk.decode(t, 20 + i, 1)[0][0])
                toks.append(t)
                rows.append(wk.read_buffer("logits", nbytes=V * 2).view(np.float16).astype(np.float32))
            if on:
                _assert_route(wk, ONE_WG, "12 steps")
            runs[on] = (toks, rows)
    for i in range(12):
        ok, why = _agree(runs[1][1][i], runs[0][1][i])
        assert ok and runs[1][0][i] == runs[0][0][i], (i, why, runs[1][0], runs[0][0])

    def state(toks):
        return (list(toks), wk.read_buffer("logits").copy(), wk.read_buffer("kcache", layer=1).copy(), wk.read_buffer("vcache", layer=1).copy())

    with _Switch(1):
        for p0, m in ((40, 30), (100, 40), (250, 20)):
            wk.reset()
            tok = int(wk.forward(prompt[:p0], 0))
            whole = state(wk.decode(tok, p0, m)[0])
            _assert_route(wk, ONE_WG, ("whole call", p0, m))
            wk.reset()
            assert int(wk.forward(prompt[:p0], 0)) == tok
            toks, t = [], tok
            for i in range(m):
                t = int(wk.decode(t, p0 + i, 1)[0][0])
                toks.append(t)
            single = state(toks)
            assert whole[0] == single[0], ("tokens", p0, m)
            assert all(np.array_equal(a, b) for a, b in zip(whole[1:], single[1:])), ("logits / last-layer caches", p0, m)
    batch = {}
    for on in (0, 1):
        with _Switch(0):                        # (the prompts the same way both times: only the batched step sees `on`)
            wk.kv_slots(2)
            for slot in (0, 1):
                wk.select_kv(slot)
                wk.forward(prompt[slot:slot + 9], 0)
        with _Switch(on):
            batch[on] = wk.decode_batch([5, 6], [9, 9], [0, 1]).tolist()
    assert batch[0] == batch[1]
    wk.close()


def test_sampled_generate_is_reached(tmp_path):
    """device_sampler on a 256-wide model: Generate of a seeded top_k query returns the tokens of the Infer / Commit loop (without the
    fused step the call is refused: "the fused decode step does not cover this model")"""
    s = dict(fx.SHAPE, **SHAPES["2over1"])
    with _Switch(0):                            # (Init sets the process-wide switch from the .ini key: put back on the way out)
        engines = []
        for name, sampler in (("gen", True), ("loop", False)):
            ini, _ = fx.write_model_dir(str(tmp_path / name), fmt="llama2.c", wd="Q4", kvd="F16", ret="false", ctx=64, s=s)
            keys = "attention_mfma_heads = true\ndevice_sampling_pool = true\n" + ("device_sampler = true\n" if sampler else "")
            text = open(ini).read().replace("return_output_tensors = false", "return_output_tensors = false\n" + keys)
            open(ini, "w").write(text)
            engines.append(InferenceEngine.from_ini(ini))
        gen, loop = engines
        assert gen.model_info("device_sampler") == 1
        prompt = [int(t) for t in np.random.default_rng(5).integers(3, 1000, 7)]
        qa = gen.add_query(prompt, strategy="top_k", seed=77)
        qb = loop.add_query(prompt, strategy="top_k", seed=77)
        assert qa > 0 and qb > 0, (gen._err(), loop._err())
        got, _ = gen.generate(qa, 16)
        want = []
        for _ in range(16):
            (q, tok), = loop.infer()
            want.append(tok)
            assert loop.commit({qb: tok})
        assert got == want and gen.model_info("device_sampled_steps") == 15
        gen.close()
        loop.close()
