"""-m gpu: the fused QKV launch after the repair of its row stream, and with the staged hand-off (csrc/ifa_decode_qkv_attn.h,
csrc/ifa_decode_attn.h; build switch IFA_QA_STAGED, off by default: the q | k rows are published before the v-only rows are multiplied;
in the UL instances the attention tail waits for q | k, runs up to P.V over the cached keys, and meets the new token's v behind a second
wait, where it writes the V row and adds the last term of one P.V chain).  Every test here holds for the library as built and for one
built with -DIFA_QA_STAGED=1 (run on MI355X with both: 38 passed each time together with tests/test_gpu_fused_attn.py and the wait tests).

  * bit identity of the fused step with the five-launch step (fuse_attn 0): token ids of every step, the last step's logits, the K and V
    cache rows of every layer -- in the UL instance (calls whose reach is above 128: positions 0 .. 300 as steps of ONE call, i.e. with
    the new row inside the 256-row entry bucket and, from 256 on, past it, where the term of key `pos` sits in the batch loop's
    sequence) and in the non-UL instances (reach <= 64 and <= 128).  Both geometries the launch has kernels for (32 kv heads: 6 / 7 rows
    per wave, 8 workgroups per kv group; 8 kv heads: 3 / 4 rows per wave, 32 workgroups), Q4_B32T1A and Q3H_B64T1 weights, F16 and
    Q8_B32T2 caches.  The planned route is asserted through Worker.decode_route().
  * the new V row and the term of key `pos`: the step's own key holds >= 0.9 of every head's weight over cached rows whose values
    look nothing like the step's v, at positions 1 (64-row bucket), 130 (UL, the row inside the bucket) and 257 (UL, past it).  The
    output is held to the bounds of tests/decode_attn_util.py (oracle.attention and float64); the test first shows that a tail which
    skipped, doubled or mis-paired that term would miss the float64 bound by >= 5 x (U.SENSITIVITY); the factor is printed.
  * the call counter in the granules' tag: 3 calls x 4 steps give the ids, logits and caches of one 12-step call."""
import numpy as np
import pytest

from inferflow_amd import dtypes as dt, synth
from tests import decode_attn_util as U

pytestmark = pytest.mark.gpu
TOK = 11
F16, Q8 = dt.F16, dt.Q8_B32T2
POSITIONS = (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 300)
GEOS = {"kv32": dict(kv_heads=32, rw=6), "kv8": dict(kv_heads=8, rw=3)}       # Llama-2-7B / Mixtral mapping of rows to workgroups
COMBOS = [(g, w, k) for g in GEOS for w in (dt.Q4_B32T1A, dt.Q3H_B64T1) for k in (F16, Q8)]
IDS = ["%s-%s-%s" % (g, "q4" if w == dt.Q4_B32T1A else "q3h", "kvf16" if k == F16 else "kvq8") for g, w, k in COMBOS]


_WORKERS = {}         # one two-layer model per (geometry, weights, cache), shared by the tests of this file


def _build(geo, wd, kvd, layers=2, max_ctx=320):
    if (geo, wd, kvd) in _WORKERS:
        return _WORKERS[(geo, wd, kvd)]
    wk, _, s = synth.build("llama2_7b", wd, kvd, max_ctx=max_ctx, layers=layers, ffn=1024, vocab=1000, kv_heads=GEOS[geo]["kv_heads"])
    ok, why = wk.fused_supported()
    assert ok, why
    wk.set_option("attn_split_ctx", 0)          # one workgroup per head in every run
    _WORKERS[(geo, wd, kvd)] = (wk, s)
    return wk, s


def _state(wk, s, toks):
    caches = [wk.read_buffer(n, layer=l).copy() for l in range(s["layers"]) for n in ("kcache", "vcache")]
    return [int(t) for t in toks], wk.read_buffer("logits").copy(), caches


def _call(wk, s, steps, fuse, route=None):
    wk.set_option("fuse_attn", fuse)
    wk.reset()
    toks, _ = wk.decode(TOK, 0, steps)
    if route is not None:
        got = wk.decode_route()
        assert {k: got[k] for k in route} == route, (got, route)
    return _state(wk, s, toks)


def _same(a, b, what):
    assert a[0] == b[0], "token ids differ (%s): first at step %d" % (what, next(i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y))
    assert np.array_equal(a[1], b[1]), "last logits differ (%s)" % what
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        assert np.array_equal(x, y), "%s cache of layer %d differs (%s)" % ("KV"[i % 2], i // 2, what)


@pytest.mark.parametrize("geo,wd,kvd", COMBOS, ids=IDS)
def test_ul_instance_is_bit_identical_to_the_five_launch_step(geo, wd, kvd):
    """positions 0 .. 300 as the steps of one call (reach 301: the 256-row bucket with unloaded heads for every step)"""
    wk, s = _build(geo, wd, kvd)
    steps = max(POSITIONS) + 1
    ref = _call(wk, s, steps, 0, dict(kind="one_workgroup"))
    got = _call(wk, s, steps, 1, dict(kind="fused_tail", pb=256, ul=1, rw=GEOS[geo]["rw"], kt=int(kvd == F16)))
    _same(got, ref, "reach %d" % steps)
    # the listed positions one by one, for the message: row p of every cache is the step's own
    rb = U.kv_row_bytes(kvd, s["kv_heads"] * s["head_dim"])
    for p in POSITIONS:
        for x, y in zip(got[2], ref[2]):
            assert np.array_equal(x[p * rb:(p + 1) * rb], y[p * rb:(p + 1) * rb]), ("cache row", p)


@pytest.mark.parametrize("geo,wd,kvd", COMBOS, ids=IDS)
def test_non_ul_instances_are_bit_identical_to_the_five_launch_step(geo, wd, kvd):
    """reach <= 64 and <= 128: the prologue waves run the tail behind their last row, with one wait, as before"""
    wk, s = _build(geo, wd, kvd)
    for steps, pb in ((64, 64), (128, 128)):
        ref = _call(wk, s, steps, 0)
        got = _call(wk, s, steps, 1, dict(kind="fused_tail", pb=pb, ul=0, rw=GEOS[geo]["rw"]))
        _same(got, ref, "reach %d" % steps)


def _own_key_case(dqkv, p, geo, seed):
    """cached rows 0 .. p - 1 under which the step's OWN key (row p) holds >= 0.9 of every head's weight: the cached keys of a kv head
    are the shortest vectors that give each query head of its group a score log(9 p) + 4 .. 5 below the head's score of the
    step's key (U.needle_rows' solve); the cached V rows are +-6 by column and key, next to a step's v of N(0, ~1)."""
    q_rot, k_p, v_p = U.new_token_rows(dqkv, p, geo)
    q = np.asarray(q_rot).astype(np.float64).reshape(geo.heads, geo.head_dim)
    s_own = U.ref_scores_f64(q_rot, k_p[None], *geo.args(), geo.attn_kq_scale)[:, 0]
    rng = np.random.default_rng(seed)
    root = np.sqrt(float(geo.head_dim))
    K = np.zeros((p, geo.kv_heads, geo.head_dim))
    for g in range(geo.kv_heads):
        Q = q[g * geo.group:(g + 1) * geo.group]
        want = s_own[None, g * geo.group:(g + 1) * geo.group] - np.log(9.0 * p) - rng.uniform(4.0, 5.0, (p, 1))     # [p][group]
        K[:, g, :] = np.linalg.solve(Q @ Q.T, (want * root).T).T @ Q
    j = np.arange(p)
    V = np.where((j[:, None] + np.arange(geo.kv_dim)[None, :]) % 2 == 0, 6.0, -6.0)
    k_rows = np.concatenate([U.pack_rows(K.reshape(p, -1).astype(np.float16), geo.kv_dtype), k_p[None]])
    v_rows = np.concatenate([U.pack_rows(V.astype(np.float16), geo.kv_dtype), v_p[None]])
    return U.Case(geo, q_rot, k_rows, v_rows, "needle", needle=p)


@pytest.mark.parametrize("kvd", [F16, Q8], ids=["kvf16", "kvq8"])
@pytest.mark.parametrize("name", ["wide128", "wide128_kv8"])
def test_new_v_row_and_the_term_of_the_steps_own_key(name, kvd):
    geo, shape, over = U.geometry(name, kvd)
    wk, _, s = synth.build(shape, dt.Q4_B32T1A, kvd, max_ctx=320, **over)
    ok, why = wk.fused_supported()
    assert ok, why
    wk.set_option("attn_split_ctx", 0)
    wk.set_option("fuse_attn", 1)
    wk.decode(TOK, 0, 1)
    dqkv_raw = wk.read_buffer("dqkv").copy()
    dqkv = dqkv_raw.view(np.float16)
    rb = geo.row_bytes
    for p in (1, 130, 257):
        c = _own_key_case(dqkv, p, geo, 100 + p)
        w = c.weights()[:, p]
        assert w.min() >= U.NEEDLE_WEIGHT, ("weight of the step's own key", p, float(w.min()))
        # a tail that skipped / doubled the late term, or paired it with its neighbour's value, is far outside the bound
        # (skipped / doubled: the term w_p x v_p left out of, or added twice to, the sum under the SAME weights -- what a tail that
        #  lost or repeated the late fma would give; delete / swap: decode_attn_util's mutations of key p)
        term = np.concatenate([w[h] * c.v64[p].reshape(geo.kv_heads, geo.head_dim)[h // geo.group] for h in range(geo.heads)])
        faults = {"skipped": c.f64 - term, "doubled": c.f64 + term, "delete": c.mutated_f64("delete", p), "swap": c.mutated_f64("swap", p)}
        for kind, out in faults.items():
            moved = float(np.abs(out - c.f64).max())
            print("staged-own-key %s %s p %d: %s moves float64 by %.1f x the bound" % (name, "q8" if kvd == Q8 else "f16", p, kind, moved / c.tol_f64))
            assert moved >= U.SENSITIVITY * c.tol_f64, (kind, p, moved, c.tol_f64)
        wk.write_buffer("kcache", c.k_rows[:p])
        wk.write_buffer("vcache", c.v_rows[:p])
        wk.decode(TOK, p, 1)
        got = wk.decode_route()
        want = dict(kind="fused_tail", pb=64 if p < 64 else 256, ul=int(p >= 128))
        assert {k: got[k] for k in want} == want, (p, got)
        att = wk.read_buffer("att").view(np.float16).copy()
        kc = wk.read_buffer("kcache", nbytes=(p + 1) * rb).reshape(p + 1, rb)
        vc = wk.read_buffer("vcache", nbytes=(p + 1) * rb).reshape(p + 1, rb)
        assert np.array_equal(wk.read_buffer("dqkv"), dqkv_raw), ("dqkv changed", p)
        assert np.array_equal(kc[:p], c.k_rows[:p]) and np.array_equal(vc[:p], c.v_rows[:p]), ("a cached row changed", p)
        U.check_new_row(kc[p], vc[p], dqkv, p, geo)
        err = U.check_att(att, c)
        print("staged-own-key %s %s p %d: err %.3f (bound 2), d_ref %.3g" % (name, "q8" if kvd == Q8 else "f16", p, err, c.d_ref))
    wk.close()


@pytest.mark.parametrize("geo,kvd", [("kv32", F16), ("kv8", Q8)], ids=["kv32-kvf16", "kv8-kvq8"])
def test_repeated_calls_on_one_model_give_the_ids_of_one_call(geo, kvd):
    """the tag of a granule is (call counter, position): 3 calls x 4 steps against one 12-step call, both behind the same 140 steps"""
    wk, s = _build(geo, dt.Q4_B32T1A, kvd)
    wk.set_option("fuse_attn", 1)
    route = dict(kind="fused_tail", pb=256, ul=1)

    def start():
        wk.reset()
        toks, _ = wk.decode(TOK, 0, 140)
        return [int(t) for t in toks]

    head = start()
    toks, _ = wk.decode(head[-1], 140, 12)
    got = wk.decode_route()
    assert {k: got[k] for k in route} == route, got
    one = _state(wk, s, toks)
    assert start() == head
    parts, t = [], head[-1]
    for i in range(3):
        toks, _ = wk.decode(t, 140 + 4 * i, 4)
        got = wk.decode_route()
        assert {k: got[k] for k in route} == route, got
        parts += [int(x) for x in toks]
        t = parts[-1]
    _same(_state(wk, s, parts), one, "3 x 4 steps against 12")
