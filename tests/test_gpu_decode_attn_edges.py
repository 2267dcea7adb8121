"""-m gpu: the attention output of the decode step itself against the oracle's arithmetic and against plain float64 math, on every
route the engine can choose, at the contexts where those routes change behaviour.

Routes: k_dec_attn (one workgroup per head; entry buckets of 64 / 128 / 256 rows, direct loads past the bucket, K rows through the LDS
tile or straight into registers), the same body as the tail of the fused QKV launch (attn_unload 0 / 1; fuse_ffn 0 and its default,
which is 0 too: the chained FFN launch is covered by tests/test_gpu_chain.py), and k_dec_attn_scores / _pv / _combine with 8 / 16 / 32
splits, contexts shorter than the split count included, also where only the LDS forces the split (max_context_len 81920).
Every walk asserts, at the first step of each context, the route the engine planned (ifa_model_decode_route: kind, entry bucket, K tile,
unloaded heads, splits, chained launch) against the one its name claims: options alone do not prove which kernel ran (a CU mask,
disabled waits or an LDS limit change it), and the failure message shows num_cus / visible_cus / waits.

One case (tests/decode_attn_util.py has the reference, the inputs and the assertions):
  * a one-layer model; a throw-away step leaves the probe token's pre-RoPE q | k | v in "dqkv" (they depend on the token and the
    weights only -- every case checks that the buffer did not change);
  * rows 0 .. p - 1 of the K and V cache are written with the case's input (F16 rows, or oracle.quantize_act_q8 rows), one step runs
    at position p, and "att", "attq" and both caches are read back;
  * att against oracle.attention within 6e-3 x max(1, max|V|) and against float64 within max(2 x d_ref, one F16 ulp at max|out|),
    d_ref = max|oracle.attention - float64| of the same case;
  * cache row p against the reference's row (F16: one ulp of the element, unrotated columns and the V row bit-equal; Q8: codes +-1,
    scales 0.002); the number of values that differ is printed per walk;
  * attq, on every head size made of whole 32-blocks, = oracle.quantize_act_q8 of the device's own att, bit for bit;
  * rows 0 .. p - 1 byte-identical to what was written.
Every route stores att (the fused launch too: its granules carry q | k | v only), so the same assertions hold on all of them.
Inputs per context: dense N(0, 1) rows; flat (every key ~1 / n, a signature +-A per V row); needle (one probed key holds >= 0.9 of the
weight of every head of its kv group), one case per probed key.  The CPU test (tests/test_decode_attn_ref_cpu.py) shows that losing, doubling
or mis-pairing any probed key moves the float64 output by >= 5 x the float64 tolerance, and that the assertions used here reject
those mutations of the oracle's output.

Measured on MI355X, err = max|att - float64| / max(d_ref, half an F16 ulp at max|out|); the bound is 2.  The median of EVERY route
is 1.000: on most inputs the device's output is the oracle's bit for bit, so its distance from float64 is d_ref itself.  Worst per route:
  one workgroup   head_dim 32: 1.078 (F16, attn_kt 0 and 1), 1.011 (Q8); head_dim 64: 1.029 (F16, kt 0 and 1), 1.553 (Q8: dense, 640 keys);
                  head_dim 48: 1.009; head_dim 128, 32 kv heads: 1.017 (F16, kt 0 and 1), 1.009 (Q8); 8 kv heads: 1.272 (F16: dense,
                  513 keys), 1.005 (Q8); head_dim 80 / 96: 1.000
  fused QKV       1.017 (F16) and 1.009 (Q8), the same for attn_unload 0 and 1 and with and without the chained FFN launch
  split x8/16/32  head_dim 64: 1.011 (F16), 1.025 (Q8); head_dim 128: 1.017 (F16), 1.051 (Q8); the same for every split count
  variants        ALiBi 1.020 (one workgroup and split), rope_order 1 and partial_rotary 0.5: 1.000
No case needs more than 2.
Needle cases and the reference's score rounding: the reference rounds a score to F16 before the softmax (a grid of 2^-7 at a needle's
score of 8 .. 16), and the device's rotated q can differ from the host's in a last bit.  A score next to a rounding edge then lands on
the other side and the output moves by ~w (1 - w) x 2^-7 x |V needle - rest| (0.002 on these inputs), which does not fit 2 x d_ref
next to d_ref itself; a score inside its cell does not move the output at all (shown on the host:
tests/test_decode_attn_ref_cpu.py::test_a_last_bit_of_q_moves_the_output_only_across_a_score_rounding_edge).  The needle rows of an
F16 cache therefore keep their scores away from those edges (decode_attn_util.needle_rows).  Q8 rows and the ALiBi geometry cannot be
placed that finely and stay exposed: a miss of that size on one of them, after a change of the weights, is this mechanism and not a
lost key, which moves the output by >= 5 x the bound.
Cache row p against the reference's row (oracle.rope of the step's k; decode_attn_util.check_new_row).  F16: ~0.1 % of the K values
differ from the reference's bits (128-wide: 89 of 73 728 over the 18 contexts; head_dim 32: 7 of 4 608; head_dim 64: 1 of 2 304),
every one of them by ONE ulp of its own size wherever the element is at least a quarter of its rotated pair's length.  Smaller
elements, where the two products nearly cancel, are held to one ulp at the pair's length instead: measured up to 36 of their own ulp
there (128-wide, position 510) and never more than 0.125 at the pair's length.  Q8: 0 .. 3 codes per walk differ from the reference's, by one.

Remaining gap: the batched attention (decode_batch / decode_draft: k_dec_attn<.., BATCH>) is not covered here."""
import numpy as np
import pytest

from inferflow_amd import dtypes as dt, synth
from tests import decode_attn_util as U

pytestmark = pytest.mark.gpu
TOK = 11
F16, Q8 = dt.F16, dt.Q8_B32T2
KV_ID = {F16: "kvf16", Q8: "kvq8"}


def _build(name, kvd, max_ctx, **more):
    geo, shape, over = U.geometry(name, kvd)
    kw = dict(over)
    kw.update(more)
    if shape == "llama2_7b":
        wd = dt.Q4_B32T1A                                  # (every matrix is past the quantisation threshold)
    elif geo.head_dim in (48, 80, 96):
        wd = dt.F16                                        # (widths that are no multiple of every block size: F16 weights)
        kw.update(layers=1, std=0.06)
    else:
        wd = dt.Q4_B32T1A
        kw.update(layers=1, quant_threshold=0, std=0.06)
    wk, _, s = synth.build(shape, wd, kvd, max_ctx=max_ctx, **kw)
    ok, why = wk.fused_supported()
    assert ok, why                                         # (otherwise decode() would run the op-by-op step: another kernel)
    return wk, s, geo


def _report(route, stats):
    errs = sorted(s[0] for s in stats)
    worst = max(stats)
    print("decode-attn-edges %-44s %5d cases  median %.3f  worst %.3f (%s, n %d, needle %s)"
          % (route, len(stats), errs[len(errs) // 2], worst[0], worst[1], worst[2], worst[3]))


def _bucket(reach):
    return 64 if reach <= 64 else 128 if reach <= 128 else 256


def _assert_route(wk, want, where):
    got = wk.decode_route()
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not diff, "%s: planned route differs from the walk's, (got, want) = %s; the whole plan: %s (num_cus %d, visible_cus %d, waits %d)" % (
        where, diff, got, got["num_cus"], got["visible_cus"], got["waits"])


def _one_wg(geo, kt):
    """the route of k_dec_attn alone at n keys: bucketed instances and the K tile on head_dim 32 / 64 / 128 only"""
    pow2 = geo.head_dim in (32, 64, 128)
    return lambda n: dict(kind="one_workgroup", pb=_bucket(n) if pow2 else 256, kt=int(bool(kt) and pow2 and geo.kv_dtype == F16), ul=0, nsplits=0, chain=0)


def _walk(wk, geo, ns, stats, route, expect):
    """every case of every context in ns through one decode step; appends (err, family, n, needle) to stats.  expect(n): the fields of
    the planned route (Worker.decode_route) a step at n keys must show"""
    wk.decode(TOK, 0, 1)
    _assert_route(wk, expect(1), (route, "first step"))
    dqkv_raw = wk.read_buffer("dqkv").copy()
    dqkv = dqkv_raw.view(np.float16)
    emits = geo.head_dim % 32 == 0 and wk.buffer("attq")[1] > 0
    rb = geo.row_bytes
    failed, rows_seen, routes_seen, row_fig = [], set(), set(), [0, 0, 0.0, 0.0]
    for n in ns:
        p = n - 1
        for c in U.make_cases(dqkv, p, geo):
            if p:
                wk.write_buffer("kcache", c.k_rows[:p])
                wk.write_buffer("vcache", c.v_rows[:p])
            wk.decode(TOK, p, 1)
            if n not in routes_seen:         # (the route depends on the reach alone: asserted once per context)
                routes_seen.add(n)
                _assert_route(wk, expect(n), (route, n))
            att = wk.read_buffer("att").view(np.float16).copy()
            kc = wk.read_buffer("kcache", nbytes=n * rb).reshape(n, rb)
            vc = wk.read_buffer("vcache", nbytes=n * rb).reshape(n, rb)
            where = (route, c.family, n, c.needle)
            assert np.array_equal(wk.read_buffer("dqkv"), dqkv_raw), ("dqkv changed", where)
            assert np.array_equal(kc[:p], c.k_rows[:p]) and np.array_equal(vc[:p], c.v_rows[:p]), ("a cached row changed", where)
            try:
                fig = U.check_new_row(kc[p], vc[p], dqkv, p, geo)
                if n not in rows_seen:           # (row p depends on the position alone: counted once per context)
                    rows_seen.add(n)
                    row_fig = [row_fig[0] + fig[0], row_fig[1] + fig[1], max(row_fig[2], fig[2]), max(row_fig[3], fig[3])]
            except AssertionError as e:
                failed.append("%s: %s" % (route, e))
            if emits:
                U.check_attq(wk.read_buffer("attq"), att, geo.qd)
            try:
                err = U.check_att(att, c)
            except AssertionError as e:      # (every case of the walk is measured before the test fails: the message names them all)
                failed.append("%s: %s; |att - oracle| %.3g" % (route, e, float(np.abs(att.astype(np.float64) - c.orc).max())))
                continue
            stats.append((err, c.family, n, c.needle))
    if stats:
        _report(route, stats)
    if geo.kv_dtype == F16:
        print("decode-attn-edges %-44s row p: %d of %d F16 K values differ from the reference's; worst %.2f own ulp, small elements %.3f pair ulp"
              % (route, row_fig[1], row_fig[0], row_fig[2], row_fig[3]))
    else:
        print("decode-attn-edges %-44s row p: %d of %d Q8 codes differ from the reference's (by one)" % (route, row_fig[1], row_fig[0]))
    assert not failed, "%d of %d cases: %s" % (len(failed), len(failed) + len(stats), " | ".join(failed))


ONE_WG = [("mha32", F16, 0), ("mha32", F16, 1), ("mha32", Q8, 0), ("gqa64", F16, 0), ("gqa64", F16, 1), ("gqa64", Q8, 0),
          ("tiny48", F16, 0), ("wide128", F16, 0), ("wide128", F16, 1), ("wide128", Q8, 0), ("wide128_kv8", F16, 1), ("wide128_kv8", Q8, 0),
          ("hd80", F16, 0), ("hd96", F16, 0), ("hd96", Q8, 0)]


@pytest.mark.parametrize("name,kvd,kt", ONE_WG, ids=["%s-%s-kt%d" % (n, KV_ID[k], t) for n, k, t in ONE_WG])
def test_one_workgroup_per_head(name, kvd, kt):
    """k_dec_attn alone (fuse_attn 0, never split): buckets 64 / 128 / 256 by the context, rows past 256 by direct loads; attn_kt 0 / 1
    on the F16 shapes that have the LDS-transposed K path (head_dim 32 / 64 / 128)"""
    wk, s, geo = _build(name, kvd, 640)
    for k, v in (("attn_split_ctx", 0), ("fuse_attn", 0), ("attn_kt", kt)):
        wk.set_option(k, v)
    ns = U.N_ONE_WG if name not in ("hd80", "hd96") else U.N_ODD_HEADS
    stats = []
    _walk(wk, geo, ns, stats, "one-wg %s %s kt%d" % (name, KV_ID[kvd], kt), _one_wg(geo, kt))
    wk.close()


@pytest.mark.parametrize("fuse_ffn", [0, None], ids=["ffn0", "ffn_default"])
@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
def test_fused_qkv_attention_launch(kvd, fuse_ffn):
    """the attention as the tail of the QKV launch (dim 4096, head_dim 128 only): the same contexts, both mappings of the heads'
    workgroups past 128 keys (attn_unload), fuse_ffn 0 and left at its default (0: no chained FFN launch in either)"""
    wk, s, geo = _build("wide128", kvd, 640)
    wk.set_option("attn_split_ctx", 0)
    wk.set_option("fuse_attn", 1)
    if fuse_ffn is not None:
        wk.set_option("fuse_ffn", fuse_ffn)
    for unload in (1, 0):
        wk.set_option("attn_unload", unload)
        ns = U.N_ONE_WG if unload == 1 else tuple(n for n in U.N_ONE_WG if n > 128)
        route = "fused-qkv %s unload%d %s" % (KV_ID[kvd], unload, "ffn0" if fuse_ffn == 0 else "ffn-default")
        stats = []
        # (F16 rows through the K tile, attn_kt's default; unloaded heads in the 256-row bucket; 8 workgroups per kv group on 256 CUs)
        _walk(wk, geo, ns, stats, route, lambda n: dict(kind="fused_tail", pb=_bucket(n), kt=int(kvd == F16), ul=int(unload == 1 and n > 128),
                                                       nsplits=0, chain=0, rw=6))
        # the fused launch is really the one that ran: its timing entry point refuses models / option sets it does not take
        assert wk.time_kernel(7, 4) > 0.0
    wk.close()


SPLIT = [(name, kvd, nsp) for name in ("gqa64", "wide128") for kvd in (F16, Q8) for nsp in (8, 16, 32)]


@pytest.mark.parametrize("name,kvd,nsplits", SPLIT, ids=["%s-%s-%dsplits" % (n, KV_ID[k], s) for n, k, s in SPLIT])
def test_keys_split_over_workgroups(name, kvd, nsplits):
    """k_dec_attn_scores / _pv / _combine from two keys on (attn_split_ctx 1), contexts with fewer keys than splits included
    (a one-key context has reach 1 and stays on one workgroup per head -- k_dec_attn, or on the 7B widths the tail of the fused QKV
    launch: that is the route the engine takes)"""
    wk, s, geo = _build(name, kvd, 704)
    wk.set_option("attn_split_ctx", 1)
    wk.set_option("attn_nsplits", nsplits)
    route = "split %s %s x%d" % (name, KV_ID[kvd], nsplits)
    stats = []
    one_key = dict(kind="fused_tail", pb=64, kt=int(kvd == F16), ul=0) if name == "wide128" else _one_wg(geo, 1)(1)
    _walk(wk, geo, U.N_SPLIT, stats, route, lambda n: one_key if n == 1 else dict(kind="split", nsplits=nsplits, split=8, chain=0))
    wk.close()


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
def test_split_forced_by_the_lds(kvd):
    """max_context_len 81920 on the 64-wide heads: a head's score row (8656 + 2 x 81920 bytes) does not fit the 160 KiB LDS, so
    k_dec_attn_scores / _pv / _combine run from position 0 on although the threshold never asks for them (attn_split_ctx 0: split = 0),
    with 8 splits of 10240 keys (36928 bytes of LDS for the P.V launch).  The contexts are a subset of gqa64's, whose references
    tests/test_decode_attn_ref_cpu.py holds to the same bounds."""
    assert set(U.N_LDS_SPLIT) <= set(U.GEOMETRIES["gqa64"][3])
    wk, s, geo = _build("gqa64", kvd, 81920)
    wk.set_option("attn_split_ctx", 0)
    stats = []
    _walk(wk, geo, U.N_LDS_SPLIT, stats, "lds-split gqa64 %s" % KV_ID[kvd],
          lambda n: dict(kind="split", nsplits=8, split=0, split_threshold=0, lds_pv=36928, error=0, chain=0))
    wk.close()


VARIANTS = [(name, kvd, split) for name, splits in (("gqa64_alibi", (0, 1)), ("gqa64_rope1", (0,)), ("gqa64_partial", (0,)))
            for kvd in (F16, Q8) for split in splits]


@pytest.mark.parametrize("name,kvd,split", VARIANTS, ids=["%s-%s-%s" % (n, KV_ID[k], "split" if s else "onewg") for n, k, s in VARIANTS])
def test_alibi_and_rope_variants(name, kvd, split):
    """use_alibi 1 (one workgroup and split), rope_order 1, partial_rotary 0.5 on the test_gqa widths"""
    wk, s, geo = _build(name, kvd, 320)
    wk.set_option("attn_split_ctx", 1 if split else 0)
    route = "%s %s %s" % (name, KV_ID[kvd], "split" if split else "one-wg")
    stats = []
    _walk(wk, geo, U.N_VARIANTS, stats, route, (lambda n: _one_wg(geo, 1)(1) if n == 1 else dict(kind="split", nsplits=8, split=8)) if split else _one_wg(geo, 1))
    wk.close()


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
@pytest.mark.parametrize("name", ["wide128", "gqa64"])
def test_call_partitioning_is_bit_identical(name, kvd):
    """positions p0 .. p0 + m - 1 as ONE call of m steps (the call's reach fixes one entry bucket for all of them) and as m one-step
    calls (every step in the smallest bucket that holds it), across the 64 / 128 / 256 edges: tokens, final logits and the whole
    last-layer caches bit for bit -- layer 1's rows carry layer 0's attention output of every middle step"""
    geo, shape, over = U.geometry(name, kvd)
    kw = dict(over)
    kw["layers"] = 2
    if shape != "llama2_7b":
        kw.update(quant_threshold=0, std=0.06)
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=320, **kw)
    ok, why = wk.fused_supported()
    assert ok, why
    prompt = (np.arange(250, dtype=np.int32) * 7 + 3) % s["vocab"]

    def state(toks):
        return (list(toks), wk.read_buffer("logits").copy(), wk.read_buffer("kcache", layer=1).copy(), wk.read_buffer("vcache", layer=1).copy())

    for p0, m in ((40, 30), (100, 40), (250, 20)):
        wk.reset()
        tok = int(wk.forward(prompt[:p0], 0))
        whole = state(wk.decode(tok, p0, m)[0])
        kind = "fused_tail" if name == "wide128" else "one_workgroup"      # (reach <= 270: under every split threshold)
        _assert_route(wk, dict(kind=kind, pb=_bucket(p0 + m)), ("whole call", p0, m))
        wk.reset()
        assert int(wk.forward(prompt[:p0], 0)) == tok
        toks, t = [], tok
        for i in range(m):
            t = int(wk.decode(t, p0 + i, 1)[0][0])
            _assert_route(wk, dict(kind=kind, pb=_bucket(p0 + i + 1)), ("single step", p0, i))
            toks.append(t)
        single = state(toks)
        assert whole[0] == single[0], ("tokens", p0, m)
        assert np.array_equal(whole[1], single[1]), ("final logits", p0, m)
        assert np.array_equal(whole[2], single[2]) and np.array_equal(whole[3], single[3]), ("last-layer caches", p0, m)
    wk.close()
