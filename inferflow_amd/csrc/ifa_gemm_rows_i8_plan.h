// ifa_gemm_rows_i8_plan.h -- what a launch of k_gemm_rows_i8 (ifa_gemm_rows_i8.hip) runs: refusal, token tiles, 16-row weight tiles per
// workgroup, grid, LDS bytes and the K limit of the fused norm, as a pure host function (no HIP calls).  The launcher takes every run-time
// value from here; the C ABI exposes it for tests (ifa_gemm_rows_i8_plan).  docs/rows_gemm_int8.md explains the numbers.
#pragma once
#include <algorithm>
#include <cstddef>
#include "ifa_dtype.h"

namespace ifa {

constexpr int GI_THREADS = 512, GI_WAVES = 8;
constexpr int GI_TOKENS = 16;                         // most token rows of one workgroup = the N of one MFMA
constexpr int GI_NORM_K_MAX = GI_THREADS * 8;         // fused RMS norm: one 8-element chunk per thread and row (4096 columns)
constexpr size_t GI_LDS_LIMIT = 160 * 1024;           // == IFA_LDS_LIMIT (ifa_decode_route.h)
// bytes of one token row's image in LDS: K int8 codes, then xs and xsum (fp32) per 32-block; rounded to 128 and + 8 so that the 16 rows
// a B operand read touches start in different banks
constexpr size_t gi_row_stride(int nblk) { return ((size_t)nblk * 40 + 127) / 128 * 128 + 8; }
// the waves' partial sums of one weight tile: [matrix][wave][4][64] fp32
constexpr size_t gi_parts_bytes(int nmat) { return (size_t)nmat * GI_WAVES * 4 * 64 * 4; }
constexpr size_t gi_norm_bytes() { return (size_t)GI_TOKENS * GI_WAVES * 4; }      // the norm's group sums, [row][wave]
constexpr size_t gi_lds_bytes(int tokens, int nblk, int nmat) { return (size_t)tokens * gi_row_stride(nblk) + gi_parts_bytes(nmat) + gi_norm_bytes(); }

// What the decision reads.  The order of the fields is the order of ifa_gemm_rows_i8_plan's `facts` array.
struct GemmRowsI8Facts {
    int T = 0;
    int w_dtype = 0;                     // DType of the (tiled) weights
    int cols = 0;                        // K
    int nsets = 1, rows0 = 0, rows1 = 0, rows2 = 0;
    int epi = 0;                         // GmEpilogue: 0 plain, 1 residual, 2 gated pair
    int norm = 0;                        // 1: the RMS norm while the rows are staged
    int has_w1 = 1;                      // the gated pair's second matrix is there
    int num_cus = 0;
};
enum GemmRowsI8Error {
    GEMM_ROWS_I8_OK = 0,
    GEMM_ROWS_I8_ERR_T = 1,              // T outside 2..32
    GEMM_ROWS_I8_ERR_DTYPE = 2,          // not tiled Q4_B32T1A / B
    GEMM_ROWS_I8_ERR_K = 3,              // K is no whole block, or no whole group of four blocks (the (base, scale) words are read four at a time)
    GEMM_ROWS_I8_ERR_GLU = 4,            // the gated pair needs one set and w3; an epilogue the kernel does not have
    GEMM_ROWS_I8_ERR_ROWS = 5,           // not 1..3 sets, a set without rows; several sets: a set's rows % 16 != 0
    GEMM_ROWS_I8_ERR_NORM = 6,           // the fused norm past its K limit
    GEMM_ROWS_I8_ERR_LDS = 7,            // not even one quantised token row fits the LDS
};
// What a launch runs.  The order of the fields is the order of ifa_gemm_rows_i8_plan's `out` array.
struct GemmRowsI8Plan {
    int error = GEMM_ROWS_I8_OK;
    int token_tiles = 0;                 // grid.x: tiles of tokens_per_wg token rows (the last one may be ragged)
    int total_rows = 0, ntiles = 0;      // virtual rows of all sets; their 16-row tiles (gated pair: pairs of tiles)
    int tiles_per_wg = 0;                // consecutive tiles one workgroup walks (1..8)
    int grid = 0;                        // grid.y: tile groups
    int lds = 0;                         // dynamic LDS bytes
    int norm_k_max = GI_NORM_K_MAX;
    int row_stride = 0;                  // gi_row_stride
    int tokens_per_wg = 0;               // token rows one workgroup stages: as many as the LDS holds, at most 16, spread evenly over the tiles
};
constexpr int GEMM_ROWS_I8_N_FACTS = sizeof(GemmRowsI8Facts) / sizeof(int), GEMM_ROWS_I8_N_OUT = sizeof(GemmRowsI8Plan) / sizeof(int);      // 11, 10

inline GemmRowsI8Plan plan_gemm_rows_i8(const GemmRowsI8Facts &f)
{
    GemmRowsI8Plan r;
    auto refuse = [&](int e) { r = GemmRowsI8Plan(); r.error = e; return r; };
    const int rows[3] = {f.rows0, f.rows1, f.rows2};
    if (f.T < 2 || f.T > 32) return refuse(GEMM_ROWS_I8_ERR_T);
    if (f.w_dtype != Q4_B32T1A && f.w_dtype != Q4_B32T1B) return refuse(GEMM_ROWS_I8_ERR_DTYPE);
    if (f.cols <= 0 || f.cols % 128 != 0) return refuse(GEMM_ROWS_I8_ERR_K);
    if (f.epi < 0 || f.epi > 2 || (f.epi == 2 && (f.nsets != 1 || !f.has_w1))) return refuse(GEMM_ROWS_I8_ERR_GLU);
    if (f.nsets < 1 || f.nsets > 3) return refuse(GEMM_ROWS_I8_ERR_ROWS);
    for (int i = 0; i < f.nsets; i++) if (rows[i] <= 0 || (f.nsets > 1 && rows[i] % 16 != 0)) return refuse(GEMM_ROWS_I8_ERR_ROWS);
    if (f.norm != 0 && (f.norm != 1 || f.cols > GI_NORM_K_MAX)) return refuse(GEMM_ROWS_I8_ERR_NORM);
    const int nblk = f.cols / 32;
    // token rows per workgroup: what the LDS holds next to the partial sums (K = 11008: 11 rows), at most 16; more rows = more token tiles
    const int nmat = f.epi == 2 ? 2 : 1;
    if (gi_lds_bytes(1, nblk, nmat) > GI_LDS_LIMIT) return refuse(GEMM_ROWS_I8_ERR_LDS);
    const int fit = (int)std::min((size_t)GI_TOKENS, (GI_LDS_LIMIT - gi_lds_bytes(0, nblk, nmat)) / gi_row_stride(nblk));
    r.token_tiles = (f.T + fit - 1) / fit;
    r.tokens_per_wg = (f.T + r.token_tiles - 1) / r.token_tiles;
    const size_t lds = gi_lds_bytes(r.tokens_per_wg, nblk, nmat);
    for (int i = 0; i < f.nsets; i++) r.total_rows += rows[i];
    r.ntiles = (r.total_rows + 15) / 16;
    // the token tiles of a tile group are neighbours in the grid, so they run at the same time and the second one finds the weights in L2;
    // one workgroup per CU over all of them, then up to 8 tiles each, then the workgroups queue
    const int cap = std::max(1, std::max(1, f.num_cus) / r.token_tiles);
    r.tiles_per_wg = std::min(8, (r.ntiles + std::min(cap, r.ntiles) - 1) / std::min(cap, r.ntiles));
    r.grid = (r.ntiles + r.tiles_per_wg - 1) / r.tiles_per_wg;
    r.lds = (int)lds;
    r.row_stride = (int)gi_row_stride(nblk);
    return r;
}

} // namespace ifa
