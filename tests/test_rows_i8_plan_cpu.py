"""The launch plan of the int8 rows GEMM (ifa_gemm_rows_i8_plan, csrc/ifa_gemm_rows_i8_plan.h): refusals, tile cover, LDS.  No device."""
import pytest

from inferflow_amd import dtypes as dt, worker as W

LDS_LIMIT = 160 * 1024          # IFA_LDS_LIMIT (csrc/ifa_decode_route.h)
PLAIN, RESIDUAL, GLU = 0, 1, 2
# the shapes tests/test_gpu_rows_i8.py launches: (rows of the sets, epilogue)
SHAPES = (((16,), PLAIN), ((40,), PLAIN), ((40,), RESIDUAL), ((16, 16, 32), PLAIN), ((48,), GLU))


@pytest.mark.parametrize("kw, error", [
    (dict(T=1), 1), (dict(T=33), 1),
    (dict(w_dtype=dt.Q8_B32T2), 2), (dict(w_dtype=dt.Q4_B64T1), 2),
    (dict(cols=2048 + 16), 3), (dict(cols=2048 + 32), 3),
    (dict(epi=GLU, has_w1=0), 4), (dict(epi=GLU, rows=(16, 16)), 4),
    (dict(rows=(16, 24, 16)), 5), (dict(rows=(16, 0)), 5),
    (dict(norm=1, cols=4096 + 128), 6),
    (dict(T=2, cols=160 * 1024), 7),
])
def test_refusals(kw, error):
    f = dict(T=4, rows=(32,), cols=2048)
    f.update(kw)
    assert W.gemm_rows_i8_plan(**f)["error"] == error
    assert W.gemm_rows_i8_plan(4, (32,), 2048, w_dtype=dt.Q4_B32T1B)["error"] == 0
    p = W.gemm_rows_i8_plan(32, (4096,), 11008, epi=RESIDUAL)      # a long row: fewer token rows per workgroup, not a refusal
    assert (p["error"], p["token_tiles"], p["tokens_per_wg"]) == (0, 3, 11) and p["lds"] <= LDS_LIMIT


@pytest.mark.parametrize("num_cus", (256, 2))
@pytest.mark.parametrize("rows, epi", SHAPES + (((12288,), PLAIN), ((11008,), GLU)))
@pytest.mark.parametrize("K", (128, 2048, 2176, 4224))
@pytest.mark.parametrize("T", (2, 3, 16, 17, 32))
def test_cover_and_lds(T, K, rows, epi, num_cus):
    p = W.gemm_rows_i8_plan(T, rows, K, epi=epi, num_cus=num_cus)
    assert p["error"] == 0, p
    assert p["token_tiles"] == (T + 15) // 16 and p["ntiles"] == (sum(rows) + 15) // 16
    assert p["tokens_per_wg"] <= 16 and p["tokens_per_wg"] * (p["token_tiles"] - 1) < T <= p["tokens_per_wg"] * p["token_tiles"]
    # consecutive groups of tiles_per_wg tiles: the last group is not empty and none is missing
    assert 1 <= p["tiles_per_wg"] <= 8 and (p["grid"] - 1) * p["tiles_per_wg"] < p["ntiles"] <= p["grid"] * p["tiles_per_wg"]
    assert p["token_tiles"] * p["grid"] <= max(num_cus, p["token_tiles"] * ((p["ntiles"] + 7) // 8))      # one per CU until 8 tiles each
    assert p["tokens_per_wg"] * (K + K // 4) <= p["lds"] <= LDS_LIMIT and p["norm_k_max"] == 4096
