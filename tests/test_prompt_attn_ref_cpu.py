"""The float64 reference, the inputs and the assertions of the prompt-attention edge tests, checked on the host for every case of the
device matrix (tests/test_gpu_prompt_attn_edges.py; tests/prompt_attn_util.py holds all three):

  (a) the float64 reference agrees with oracle.attention within what the reference's own rounding points allow, on every query row;
  (b) every fault of prompt_attn_util.faults_of -- a probed key deleted, counted twice or paired with its neighbour's V row; a row's
      causal bound off by one in either direction at the first and last query of each 32-query group; a whole 32-key block lost or
      doubled (the last block, the block before the first query's diagonal, an odd-parity block); the two parities' sums merged without
      rescaling; the V block's columns in unpermuted order; a row receiving the result of row q_tokens - 1; the kv heads of the
      neighbouring group; the ALiBi slope of the neighbouring head -- moves the float64 value of at least one element of its row by
      >= SENSITIVITY (5) x the row's bound (where: prompt_attn_util.sensitivity_required lists the exemptions and the case that covers
      each exempt fault);
  (c) the assertions the device test applies (prompt_attn_util.check_rows) accept the oracle's output and REJECT it carrying each of
      those faults, so a kernel with one of them cannot pass.

Recorded run: docs/prompt_attention_edges.md has the counts."""
import numpy as np
import pytest

from tests import prompt_attn_util as U

SHAPES = U.device_matrix()
ROW_SHAPES = [s for b in U.ROWS_BATCHES for s in U.rows_batch_shapes(b)]
TOTALS = {"cases": 0, "faults": 0, "rejected": 0, "accepted": 0, "least": (np.inf, None)}


def _reference_bound(c, t):
    """how far the reference may sit from exact math on row t: its weights carry the F16 roundings of S (half an ulp at the largest
    score, bias included), of e and of P (2^-11 each); a relative weight error eps moves a convex mix of V by <= 4 eps max|V|; the
    output is rounded to F16 once more"""
    vis = c.count[t] > 0
    eps = 2.0 ** -10 + 0.5 * float(U.D.ulp16(np.abs(c.scores[:, t, vis]).max()))
    return 4.0 * eps * c.vmax + 0.5 * float(U.D.ulp16(np.abs(c.f64[t]).max()))


def _walk(sh):
    n_cases, n_faults, n_rej, least = 0, 0, 0, (np.inf, None)
    seen = set()
    for c in U.make_cases(sh):
        n_cases += 1
        for t in range(sh.qt):
            assert c.d_ref[t] <= _reference_bound(c, t), ("float64 reference and oracle.attention disagree", c.tag, t, c.d_ref[t], _reference_bound(c, t))
        assert U.check_rows(c.orc, c).max() <= 2.0
        for name, t, kw, j in U.faults_of(c):
            if not U.sensitivity_required(c, name, t, j):
                continue
            move = float(np.abs(U.faulty_row(c, t, kw, oracle=False) - c.f64[t]).max()) / float(c.tol_f64[t])
            assert move >= U.SENSITIVITY, ("%s (row %d, key %s) moves the float64 row by only %.2f x its bound" % (name, t, j, move), c.tag)
            if move < least[0]:
                least = (move, "%s, row %d, key %s, %s" % (name, t, j, c.tag))
            bad = c.orc.copy()
            bad[t] = U.faulty_row(c, t, kw, oracle=True)
            n_faults += 1
            try:
                U.check_rows(bad, c)
            except AssertionError:
                n_rej += 1
            else:
                TOTALS["accepted"] += 1
                raise AssertionError("the oracle's output with '%s' at row %d, key %s was accepted (%s)" % (name, t, j, c.tag))
            seen.add((name, c.family))
    TOTALS["cases"] += n_cases; TOTALS["faults"] += n_faults; TOTALS["rejected"] += n_rej
    if least[0] < TOTALS["least"][0]:
        TOTALS["least"] = least
    print("prompt-attn-ref %s: %d cases, %d faulty outputs, %d rejected, least move %.1f x bound (%s)" % (sh.id, n_cases, n_faults, n_rej, least[0], least[1]))
    return seen


@pytest.mark.parametrize("sh", SHAPES, ids=[s.id for s in SHAPES])
def test_reference_inputs_and_faults(sh):
    for settings, kind in sh.routes():          # the kernels the device test means to run on this input are the ones the plan names
        p = sh.plan(settings)
        assert p["error"] == 0 and p["kind"] == kind, (sh.id, settings, U.KIND_NAMES[kind], p)
    seen = _walk(sh)
    names = {n for n, _ in seen}
    if sh.n_ctx >= 2:
        assert {"key deleted", "key paired with its neighbour's V row"} <= names
        assert sh.alibi or "key counted twice" in names          # (under ALiBi: sensitivity_required says why not, and what answers for it)
    if sh.qt >= 2:
        assert "row of the clamped query" in names and "causal bound + 1" in names and "causal bound - 1" in names
    if sh.kind in (U.TWO_PASS64, U.TWO_PASS128) and not sh.alibi:
        assert "V block columns unpermuted" in names and "block lost" in names and "block doubled" in names
    if sh.kind in (U.TWO_PASS64, U.TWO_PASS128):
        assert "parities merged without rescaling" in names
    if sh.kv_heads > 1:
        assert "kv heads of the neighbouring group" in names
    if sh.alibi:
        assert "ALiBi slope of the neighbouring head" in names


@pytest.mark.parametrize("sh", ROW_SHAPES, ids=["rows-" + s.id for s in ROW_SHAPES])
def test_rows_of_a_batch_as_one_query_cases(sh):
    _walk(sh)


def test_totals_and_matrix_coverage():
    """(runs last in this file) every faulty output of the walk above was rejected; and the matrix reaches the edges it is meant for"""
    print("prompt-attn-ref total: %d cases, %d faulty outputs, %d rejected, %d accepted; least move %.1f x bound (%s)"
          % (TOTALS["cases"], TOTALS["faults"], TOTALS["rejected"], TOTALS["accepted"], TOTALS["least"][0], TOTALS["least"][1]))
    assert TOTALS["accepted"] == 0 and TOTALS["rejected"] == TOTALS["faults"]
    two = [s for s in U.TWO_PASS]
    assert {s.qt for s in two} >= {64, 65, 95, 96, 97, 127, 128, 129, 161} and {s.prefix for s in two} >= {0, 1, 31, 32, 33, 63, 64, 200}
    assert {(s.qt - 1) % 64 + 1 for s in two} >= {1, 31, 32, 33, 63, 64}                    # queries of the last tile
    assert {s.tile_nkb(64)[0] for s in two} >= {2, 3} and {s.tile_nkb(64)[-1] % 2 for s in two} == {0, 1}
    assert any(s.n_ctx > s.prefix + s.qt for s in two)
    lds = [s for s in U.MFMA]
    assert {s.qt for s in lds} >= {4, 5, 31, 32, 33, 63} and {s.hd for s in lds} == {32, 64, 128}
    assert {k for s in lds for k in s.tile_nkb(32)} >= {1, 4, 5, 8, 9, 12, 13}
    assert {s.n_valid(s.qt - 1) % 8 for s in lds} >= {0, 1, 7}
    for s in SHAPES:
        assert (8 in {x.heads for x in SHAPES}) and s.heads % s.kv_heads == 0
    assert {s.heads // s.kv_heads for s in two + lds} >= {1, 2, 4} and {s.heads for s in two + lds} >= {4, 6, 8}
