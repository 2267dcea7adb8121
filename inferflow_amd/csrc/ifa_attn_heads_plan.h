// ifa_attn_heads_plan.h -- the launch of k_attention_heads16 (ifa_attn_heads.hip), the prompt attention kernel on 16-wide MFMA tiles for
// head_dim 48 / 80 / 96: whether it takes a call of ifa_attention, its grid, its dynamic LDS bytes and the XCD remap of (tile, head), as a
// pure host function: no HIP call.  The launcher takes its values from the plan, the kernel takes the tile constants from here, the C ABI
// exposes it for tests (ifa_attention_heads16_plan).  plan_attention (ifa_attn_plan.h) is not touched: it keeps answering Scalar for these
// head sizes, and ifa_attention asks this plan only with ifa_attention_mfma_heads(1).
#pragma once
#include "ifa_attn_plan.h"

namespace ifa {

constexpr int H16_QT = 64;           // queries per workgroup: four waves of 16
constexpr int H16_KB = 32;           // keys per staged block
constexpr int H16_KPAD = 8;          // halfs behind a K row in the LDS (see h16_krow)
constexpr int H16_VROW = PF_VROW;    // halfs per row of the transposed V block (32 key columns + pad), as the other kernels
constexpr int H16_MIN_QUERIES = 4;   // fewer stay on k_attention, as for the other MFMA kinds

constexpr bool attn_heads16_head(int head_dim) { return head_dim == 48 || head_dim == 80 || head_dim == 96; }
// A K row of HD halfs is 6 / 10 / 12 16-byte chunks: an even count, so rows 4 apart (96: 2 apart) would start in the same banks and
// the rows of a fragment read (one 16-byte chunk per lane, same column) would collide 2-fold (96: 4-fold).  One chunk of pad makes the
// row 7 / 11 / 13 chunks -- odd -- so any 8 consecutive rows start in 8 different 16-byte bank groups of the 32 banks: conflict-free b128
// reads, and every row stays 16-byte aligned.
IFA_HD constexpr int h16_krow(int head_dim) { return head_dim + H16_KPAD; }
// [2 buffers] K block [32][h16_krow] halfs, then [2 buffers] V block transposed [head_dim][H16_VROW] halfs
constexpr int attn_heads16_lds(int head_dim) { return 2 * H16_KB * h16_krow(head_dim) * 2 + 2 * head_dim * H16_VROW * 2; }

enum AttnHeads16Error {              // 0 .. 5: AttnPlanError of plan_attention on the same facts
    ATTN16_ERR_HEAD_SIZE = 6,        // head_dim is not 48 / 80 / 96
    ATTN16_ERR_FEW_QUERIES = 7,      // q_tokens < 4
    ATTN16_ERR_ROWS_MODE = 8,        // ifa_attention_rows stays on k_attention
};
// The order of the fields is the order of ifa_attention_heads16_plan's `out` array.
struct AttnHeads16Plan {
    int error = ATTN_OK;
    int q_per_wg = 0;
    int grid_x = 0, grid_y = 0;      // (query tiles, heads)
    int lds = 0;                     // dynamic LDS bytes
    int xcd_remap = 0;               // the kernel maps (tile, head) so that an XCD keeps an eighth of the heads
};
constexpr int ATTN16_N_OUT = sizeof(AttnHeads16Plan) / sizeof(int);      // 6

inline AttnHeads16Plan plan_attention_heads16(const AttnFacts &f)
{
    AttnHeads16Plan r;
    auto refuse = [&](int e) { r = AttnHeads16Plan(); r.error = e; return r; };
    if (f.rows_mode) return refuse(ATTN16_ERR_ROWS_MODE);
    const AttnPlan base = plan_attention(f);             // dtype, heads, the cache row of whole 32-blocks, shape, length
    if (base.error != ATTN_OK) return refuse(base.error);
    if (!attn_heads16_head(f.head_dim)) return refuse(ATTN16_ERR_HEAD_SIZE);
    if (f.q_tokens < H16_MIN_QUERIES) return refuse(ATTN16_ERR_FEW_QUERIES);
    r.q_per_wg = H16_QT;
    r.grid_x = (f.q_tokens + H16_QT - 1) / H16_QT;
    r.grid_y = f.heads;
    r.lds = attn_heads16_lds(f.head_dim);
    r.xcd_remap = f.heads % 8 == 0;
    return r;
}

} // namespace ifa
