"""The float64 reference, the inputs and the assertions of the decode-attention edge tests, checked on the host for every case of the
GPU matrix (tests/test_gpu_decode_attn_edges.py; the q | k | v of the probe token are N(0, 1) stand-ins here, the inputs are built
relative to q either way):

  (a) the float64 reference agrees with oracle.attention and oracle.rope within what the reference's own rounding points allow;
  (b) the sensitivity condition: deleting, duplicating or mis-pairing (swap with the neighbour's value) any probed key moves the
      float64 output by >= 5 x the float64 tolerance of the case (exemptions: Case.sensitivity_required);
  (c) d_ref = max|oracle.attention - float64| of every case, the figure the GPU bound 2 x d_ref rests on, is measured and printed;
  (d) the assertions the GPU test applies to the device's output (decode_attn_util.check_att) accept the oracle's output and REJECT
      it after each mutation -- one key dropped, doubled, paired with its neighbour's value, the kv heads of another group -- so a
      kernel with one of those faults cannot pass.

Recorded run (worst over the matrix): least sensitivity 14.3 x the tolerance (dense, head_dim 32, Q8 cache, 63 keys), 18.8 x for the
needle family without ALiBi and 7.0 x with it; d_ref up to 0.016 (flat, 128-wide, Q8 cache) and 0.045 under ALiBi (flat, 257 keys);
the oracle's rotation within 0.60 ulp of float64; about 15 000 mutated outputs rejected, none accepted."""
import numpy as np
import pytest

from inferflow_amd import dtypes as dt
from tests import decode_attn_util as U

CASES = [(name, kvd) for name, (_, _, kvds, _) in U.GEOMETRIES.items() for kvd in kvds]
IDS = ["%s-%s" % (n, "kvf16" if k == dt.F16 else "kvq8") for n, k in CASES]


def _score_magnitude(c):
    return float(np.abs(c.scores).max())


def _reference_bound(c):
    """how far the reference may sit from exact math: its weights carry the F16 roundings of S (half an ulp at the largest score,
    bias included), of e and of P (2^-11 each); a relative weight error eps moves a convex mix of V by <= 2 eps max|V - out|
    <= 4 eps max|V|; the output is rounded to F16 once more"""
    eps = 2.0 ** -10 + 0.5 * float(U.ulp16(_score_magnitude(c)))
    return 4.0 * eps * c.vmax + 0.5 * float(U.ulp16(np.abs(c.f64).max()))


@pytest.mark.parametrize("name,kvd", CASES, ids=IDS)
def test_float64_reference_inputs_and_assertions(name, kvd):
    geo, _, _ = U.geometry(name, kvd)
    ns = U.GEOMETRIES[name][3]
    dqkv = U.synthetic_dqkv(geo, 11)
    worst_s, worst_d, n_cases, n_rejected = (np.inf, None), (0.0, None), 0, 0
    for n in ns:
        for c in U.make_cases(dqkv, n - 1, geo):
            n_cases += 1
            tag = (c.family, n, c.needle)
            # (a) + (c)
            assert c.d_ref <= _reference_bound(c), ("float64 reference and oracle.attention disagree", tag, c.d_ref, _reference_bound(c))
            if c.d_ref > worst_d[0]:
                worst_d = (c.d_ref, tag)
            if c.family != "needle" or c.needle == 0:      # (the needle cases share their background's scores: the shortcut against the plain call)
                direct = U.ref_attention_f64(c.q_rot, c.k_rows, c.v_rows, *geo.args(), geo.attn_kq_scale, bool(geo.use_alibi), 0, geo.heads)
                assert np.abs(direct - c.f64).max() <= 1e-12 * max(1.0, c.vmax), ("shared-background reference differs from a fresh one", tag)
            if c.family == "flat":
                raw = U.ref_scores_f64(c.q_rot, c.k_rows[:n - 1], *geo.args(), geo.attn_kq_scale)          # (without the ALiBi bias)
                assert np.abs(raw).max() <= U.FLAT_SCORE, ("flat family: a cached key's score", tag, float(np.abs(raw).max()))
            if c.family == "needle" and kvd == dt.F16 and not geo.use_alibi:
                # the needle's scores keep a quarter of a half-cell from the reference's rounding edges: at scores of 8 .. 16 that is
                # 2^-10, the size of what a last-bit difference in one element of the rotated q moves a score by (measured: <= 0.61)
                sj = c.scores[:, c.needle]
                off = np.abs(sj - np.float16(sj).astype(np.float64)) / (U.ulp16(sj) / 2)
                assert off.max() <= 0.75, ("needle score next to a rounding edge of the reference", tag, float(off.max()))
            # (b)
            s = c.sensitivity()
            if c.sensitivity_required():
                assert s >= U.SENSITIVITY, ("a mutation of a probed key moves the float64 output by only %.2f x the tolerance" % s, tag)
                if s < worst_s[0]:
                    worst_s = (s, tag)
            # (d) the GPU assertions on the oracle's own output, and on its mutations
            assert U.check_att(c.orc, c) <= 2.0
            with pytest.raises(AssertionError):
                U.check_att(c.mutated_oracle("wrong_head", 0), c)
            n_rejected += 1
            if c.sensitivity_required():
                for j in c.probes():
                    for kind in c.mutation_kinds(j):
                        with pytest.raises(AssertionError):
                            U.check_att(c.mutated_oracle(kind, j), c)
                        n_rejected += 1
    print("decode-attn-ref %s: %d cases, least sensitivity %.1f x tolerance %s, largest d_ref %.2g %s, %d mutations rejected"
          % (name, n_cases, worst_s[0], worst_s[1], worst_d[0], worst_d[1], n_rejected))


@pytest.mark.parametrize("name,kvd", CASES, ids=IDS)
def test_float64_rope_agrees_with_the_oracle(name, kvd):
    """both rope_order values, partial rotary, every position the matrix uses: the oracle's F16 row is within one F16 ulp of the
    unrounded float64 rotation (its own rounding is half an ulp; its angle is a float32 product: decode_attn_util.rope_tolerance)"""
    geo, _, _ = U.geometry(name, kvd)
    x = U.synthetic_dqkv(geo, 5)[:geo.qd].reshape(geo.heads, geo.head_dim)
    worst = 0.0
    for n in U.GEOMETRIES[name][3]:
        exact = U.ref_rope_f64(x, n - 1, geo.theta, geo.rope_order, geo.partial_rotary)
        got = U.oracle_rope(x, n - 1, geo).astype(np.float64)
        tol = U.rope_tolerance(x, geo.rope_order, geo.partial_rotary)
        assert (np.abs(got - exact) <= tol).all(), (name, n, float((np.abs(got - exact) / tol).max()))
        worst = max(worst, float((np.abs(got - exact) / tol).max()))
        if geo.partial_rotary < 1.0 and geo.rope_order == 2:
            r = int(geo.head_dim * geo.partial_rotary + 0.5)
            assert np.array_equal(exact[:, r:], x[:, r:].astype(np.float64))
    print("decode-attn-ref rope %s: worst |oracle - float64| = %.2f ulp at the pair's length" % (name, worst))


def test_alibi_slopes_and_head_map_follow_the_definition():
    # 8 heads: 2^-1 .. 2^-8; 6 heads (not a power of two): 4 slopes of the 4-head series, then the odd members of the 8-head series
    assert np.allclose(U.alibi_slopes(8), 2.0 ** -np.arange(1, 9))
    assert np.allclose(U.alibi_slopes(6), [2.0 ** -2, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8, 2.0 ** -1, 2.0 ** -3])
    assert np.allclose(U.alibi_slopes(2, base_head=2, total_heads=4), [2.0 ** -6, 2.0 ** -8])
    assert list(U.kv_head_of(8, 2)) == [0, 0, 0, 0, 1, 1, 1, 1] and list(U.kv_head_of(4, 4)) == [0, 1, 2, 3]
    assert U.probed_keys(700)[:3] == [0, 1, 56] and U.probed_keys(700)[-1] == 699 and 519 in U.probed_keys(700)
    assert U.probed_keys(1) == [0] and U.probed_keys(0) == []


def test_q8_rows_dequantise_as_scale_times_code():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 2, (5, 64)).astype(np.float16)
    rows = U.pack_rows(x, dt.Q8_B32T2)
    b = rows.reshape(5, 2, 34)
    want = b[:, :, 2:].view(np.int8).astype(np.float64) * b[:, :, :2].copy().view(np.float16).astype(np.float64)
    assert np.array_equal(U.rows_f64(rows, dt.Q8_B32T2, 64), want.reshape(5, 64))
    assert np.abs(U.rows_f64(rows, dt.Q8_B32T2, 64) - x.astype(np.float64)).max() <= np.abs(x).max() / 127 * 0.51 + 1e-3
    assert np.array_equal(U.rows_f64(U.pack_rows(x, dt.F16), dt.F16, 64), x.astype(np.float64))


def _oracle_score(q16, k16, head_dim):
    """the reference's score of one key before its F16 rounding: float32 products added in d order, times 1 / sqrt(head_dim)"""
    acc = np.float32(0)
    for a, b in zip(q16.astype(np.float32), k16.astype(np.float32)):
        acc = np.float32(acc + np.float32(a * b))
    return np.float32(np.float32(1 / np.sqrt(np.float32(head_dim))) * acc)


def test_a_last_bit_of_q_moves_the_output_only_across_a_score_rounding_edge():
    """Why the needle rows keep their scores away from the reference's F16 rounding edges (decode_attn_util.needle_rows).  The reference
    rounds a score to F16 before the softmax; a device whose rotated q differs from the host's in the last bit of one element (its own
    powf / cosf) moves a score by <= ~5e-4.  On the host, with oracle.attention: flipping the last bit of any single element of q
    leaves the output of a needle case bit for bit alone when the needle's score sits inside its rounding cell, and moves it by about
    w (1 - w) x one F16 score step x |V needle - rest| -- more than 2 x d_ref leaves room for next to d_ref -- exactly for those flips
    that carry the score across an edge when it sits next to one.  Rows that cannot be placed (Q8 blocks, the ALiBi geometry) stay
    exposed to this: a miss of about that size on such a case is this mechanism, not a lost key (which moves the output >= 5 x the bound)."""
    geo, _, _ = U.geometry("tiny48", dt.F16)
    dqkv = U.synthetic_dqkv(geo, 11)
    j, h, hd = 1, 0, geo.head_dim
    c = [c for c in U.make_cases(dqkv, 254, geo, families=("needle",)) if c.needle == j][0]
    w = float(c.weights()[h, j])
    predicted = w * (1 - w) * float(U.ulp16(c.scores[h, j])) * 4.0            # (V needle = +-4, the rest mixes to ~0)

    def flips(k_rows):
        base = U.oracle_attention(c.q_rot, k_rows, c.v_rows, geo, kv_groups=(0, 1))
        kj = k_rows[j].view(np.float16)[:hd]
        s0 = _oracle_score(c.q_rot[h], kj, hd)
        crossing, other = [], []
        for d in range(hd):
            q = c.q_rot.copy()
            q.view(np.uint16)[h, d] ^= 1
            jump = float(np.abs(U.oracle_attention(q, k_rows, c.v_rows, geo, kv_groups=(0, 1)) - base).max())
            (crossing if np.float16(_oracle_score(q[h], kj, hd)) != np.float16(s0) else other).append(jump)
        return crossing, other

    crossing, other = flips(c.k_rows)
    assert not crossing and max(other) == 0.0, (len(crossing), max(other))
    # the same case with the needle's row scaled by <= 6e-4 until its score sits next to an edge
    k16, best = c.k_rows[j].view(np.float16).astype(np.float64), None
    for t in np.linspace(1 - 6e-4, 1 + 6e-4, 400):
        kr = (k16 * t).astype(np.float16)
        s = _oracle_score(c.q_rot[h], kr[:hd], hd)
        dist = abs(abs(float(s) - float(np.float16(s))) - float(U.ulp16(s)) / 2)
        if best is None or dist < best[0]:
            best = (dist, kr)
    k_edge = c.k_rows.copy()
    k_edge[j] = best[1].view(np.uint8)
    crossing, other = flips(k_edge)
    print("decode-attn-ref edge: %d of %d last-bit flips cross the edge, output jump %.5f .. %.5f (predicted %.5f, d_ref %.5f, bound %.5f); "
          "the other flips move it by %.5f" % (len(crossing), hd, min(crossing), max(crossing), predicted, c.d_ref, c.tol_f64, max(other)))
    assert crossing and min(crossing) >= 0.5 * predicted and max(crossing) <= 2.0 * predicted
    assert max(other) == 0.0
    assert max(crossing) > c.d_ref          # (larger than the reference's own distance: on top of it, it does not fit 2 x d_ref in general)
