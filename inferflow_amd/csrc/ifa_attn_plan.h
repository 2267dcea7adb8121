// ifa_attn_plan.h -- which of the prompt attention kernels (ifa_attn.hip) a call of ifa_attention / ifa_attention_rows runs -- the kind,
// queries per workgroup, grid, dynamic LDS bytes, the score workspace of the global-tile variant, the XCD remap of (tile, head) -- as a
// pure host function: no HIP call.  The launchers take their choice and their run-time values from the plan; the kernels take the tile
// constants from here; the C ABI exposes it for tests (ifa_attention_plan).  The measurements behind every number are in ifa_attn.hip.
#pragma once
#include <cstddef>
#include "ifa_dtype.h"

namespace ifa {

constexpr int PF_QT = 32;            // queries per workgroup of the staged kernel (k_attention_mfma)
constexpr int PF_VROW = 40;          // halfs per row of the transposed V block (32 keys + pad: conflict-free b128 reads)
constexpr int F2_QT = 128;           // queries per workgroup of k_attention_2pass (k_attention_2pass_ks: F2K_QT)
constexpr int F2K_QT = 64;
constexpr int F2_VROW = 40;          // halfs per row of the transposed V block (32 key columns + pad)
constexpr int PF_LDS_LIMIT = 150 * 1024;     // the [32 x keys] score tile stays in the LDS up to here (of 160 KiB), else the global workspace
constexpr int ATTN_MAX_CTX = 65536, ATTN_MAX_QUERIES = 65535;

IFA_HD inline int pf_nkp(int n_keys) { return (n_keys + 31) / 32 * 32 + 8; }     // halfs per row of the score tile

constexpr bool attn_mfma_head(int head_dim) { return head_dim == 32 || head_dim == 64 || head_dim == 128; }
constexpr bool attn_2pass_head(int head_dim) { return head_dim == 64 || head_dim == 128; }
inline size_t attn_scalar_lds(int n_ctx) { return (((size_t)n_ctx * 2 + 15) & ~(size_t)15) + 64; }      // S[n_ctx] halfs, then the 8 partial results
inline size_t attn_mfma_lds(int n_ctx, int head_dim) { return (size_t)PF_QT * pf_nkp(n_ctx) * 2 + (size_t)head_dim * PF_VROW * 2 + 64; }     // score tile + V block
inline size_t attn_ws_lds(int head_dim) { return (size_t)head_dim * PF_VROW * 2 + 64; }                 // the V block alone
inline size_t attn_2pass64_lds(int head_dim) { return (size_t)4 * 32 * head_dim * 2 + (size_t)4 * head_dim * F2_VROW * 2; }    // [2 stages][2 parities] K, then V

enum AttnKind {
    ATTN_SCALAR = 0,                 // k_attention: one workgroup per (head, query)
    ATTN_MFMA_LDS = 1,               // k_attention_mfma<.., SG = false>
    ATTN_MFMA_WORKSPACE = 2,         // k_attention_mfma<.., SG = true>
    ATTN_TWO_PASS64 = 3,             // k_attention_2pass_ks
    ATTN_TWO_PASS128 = 4,            // k_attention_2pass
};

// What the decision reads.  The order of the fields is the order of ifa_attention_plan's `facts` array.
struct AttnFacts {
    int kv_dtype = F16;
    int n_ctx = 0, q_tokens = 0, prefix_len = 0;     // rows mode: the longest context of the batch, its rows, ignored
    int heads = 0, kv_heads = 0, head_dim = 0;
    int two_pass_min = 64;           // ifa_attention_two_pass_min as it is stored (never: 1 << 30)
    int two_pass_min_keys = 1 << 30; // ifa_attention_two_pass_min_keys
    int rows_mode = 0;               // ifa_attention_rows: every row one query on its own cache
};
enum AttnPlanError {
    ATTN_OK = 0,
    ATTN_ERR_DTYPE = 1,              // the cache is neither F16 nor Q8_B32T2
    ATTN_ERR_HEADS = 2,              // heads, kv_heads < 1 or heads % kv_heads != 0
    ATTN_ERR_HEAD_DIM = 3,           // head_dim < 1 or a cache row that is no whole 32-blocks
    ATTN_ERR_SHAPE = 4,              // n_ctx, q_tokens < 1 or prefix_len < 0 (rows mode: rows, longest context < 1)
    ATTN_ERR_TOO_LONG = 5,           // n_ctx > 65536 or q_tokens > 65535
};
// What a call runs.  The order of the fields is the order of ifa_attention_plan's `out` array (ws_bytes: two ints, low half first).
struct AttnPlan {
    int error = ATTN_OK;
    int kind = ATTN_SCALAR;
    int q_per_wg = 0;
    int grid_x = 0, grid_y = 0;
    int lds = 0;                     // dynamic LDS bytes of the launch (k_attention_2pass: 0, its tiles are static)
    int sg_nkp = 0;                  // row stride of the score tiles in the workspace, halfs
    int xcd_remap = 0;               // the kernel maps (tile, head) so that an XCD keeps an eighth of the heads
    long long ws_bytes = 0;          // [heads][tiles][32][sg_nkp] halfs
};
constexpr int ATTN_N_FACTS = sizeof(AttnFacts) / sizeof(int), ATTN_N_OUT = sizeof(AttnPlan) / sizeof(int);      // 10, 10

inline const char *attn_plan_error_text(int e)
{
    switch (e) {
    case ATTN_ERR_DTYPE: return "kv dtype";
    case ATTN_ERR_HEADS: return "heads / kv_heads";
    case ATTN_ERR_HEAD_DIM: return "head_dim";
    case ATTN_ERR_SHAPE: return "n_ctx / q_tokens / prefix";
    case ATTN_ERR_TOO_LONG: return "context too long for the op-level kernel";
    default: return "";
    }
}

inline AttnPlan plan_attention(const AttnFacts &f)
{
    AttnPlan r;
    auto refuse = [&](int e) { r = AttnPlan(); r.error = e; return r; };
    if (f.rows_mode) {               // (the rows entry checks nothing else: the engine hands it its own geometry)
        if (f.q_tokens < 1 || f.n_ctx < 1) return refuse(ATTN_ERR_SHAPE);
        r.kind = ATTN_SCALAR; r.q_per_wg = 1; r.grid_x = f.heads; r.grid_y = f.q_tokens; r.lds = (int)attn_scalar_lds(f.n_ctx);
        return r;
    }
    if (f.kv_dtype != F16 && f.kv_dtype != Q8_B32T2) return refuse(ATTN_ERR_DTYPE);
    if (f.heads < 1 || f.kv_heads < 1 || f.heads % f.kv_heads != 0) return refuse(ATTN_ERR_HEADS);
    if (f.head_dim < 1 || ((long long)f.kv_heads * f.head_dim) % 32 != 0) return refuse(ATTN_ERR_HEAD_DIM);
    if (f.n_ctx < 1 || f.q_tokens < 1 || f.prefix_len < 0) return refuse(ATTN_ERR_SHAPE);
    if (f.n_ctx > ATTN_MAX_CTX || f.q_tokens > ATTN_MAX_QUERIES) return refuse(ATTN_ERR_TOO_LONG);
    auto tiles = [&](int qt) { return (f.q_tokens + qt - 1) / qt; };
    const bool wide = f.q_tokens >= F2_QT && f.n_ctx >= f.two_pass_min_keys;      // the 128-query variant is asked for
    r.grid_y = f.heads;
    r.xcd_remap = f.heads % 8 == 0;
    if (f.q_tokens >= f.two_pass_min && attn_2pass_head(f.head_dim)) {
        // chunks of >= 64 queries: 64 queries per workgroup, the key blocks split over wave pairs; or one wave per 32 queries of 128
        r.kind = wide ? ATTN_TWO_PASS128 : ATTN_TWO_PASS64;
        r.q_per_wg = wide ? F2_QT : F2K_QT;
        r.grid_x = tiles(r.q_per_wg);
        r.lds = wide ? 0 : (int)attn_2pass64_lds(f.head_dim);
        return r;
    }
    if (f.q_tokens >= 4 && attn_mfma_head(f.head_dim)) {
        // the staged kernel: the [32 x n_keys] score tile in the LDS while it fits (~2300 keys), else in the global workspace
        const bool fits = attn_mfma_lds(f.n_ctx, f.head_dim) <= (size_t)PF_LDS_LIMIT;
        r.kind = fits ? ATTN_MFMA_LDS : ATTN_MFMA_WORKSPACE;
        r.q_per_wg = PF_QT;
        r.grid_x = tiles(PF_QT);
        r.lds = (int)(fits ? attn_mfma_lds(f.n_ctx, f.head_dim) : attn_ws_lds(f.head_dim));
        if (!fits) {
            r.sg_nkp = pf_nkp(f.n_ctx);
            r.ws_bytes = (long long)f.heads * r.grid_x * PF_QT * (long long)r.sg_nkp * 2;
        }
        return r;
    }
    r.kind = ATTN_SCALAR; r.q_per_wg = 1; r.grid_x = f.heads; r.grid_y = f.q_tokens; r.lds = (int)attn_scalar_lds(f.n_ctx); r.xcd_remap = 0;
    return r;
}

} // namespace ifa
