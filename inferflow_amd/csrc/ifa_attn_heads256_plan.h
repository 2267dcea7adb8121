// ifa_attn_heads256_plan.h -- the launch of prompt attention for head_dim 256 (Gemma) on the matrix cores: whether it takes a call of
// ifa_attention, its grid, its dynamic LDS bytes and the XCD remap of (tile, head), as a pure host function: no HIP call.  The kernel is
// k_attention_heads16<256, Q8> (ifa_attn_heads.hip): of the two designs measured -- that template at 256 and a kernel of 128 queries per
// workgroup on 32 x 32 tiles with one wave per SIMD -- the 16-wide tiles were faster at every size (docs/prompt_attention_heads256.md).
// The launcher takes its values from the plan, the C ABI exposes it for tests (ifa_attention_heads256_plan).  plan_attention
// (ifa_attn_plan.h) and plan_attention_heads16 are not touched: they keep answering Scalar and "head size" for 256, and ifa_attention asks
// this plan only with ifa_attention_mfma_heads(1).
#pragma once
#include "ifa_attn_heads_plan.h"

namespace ifa {

constexpr int H256_HD = 256;         // the one head size
constexpr int H256_QT = H16_QT;      // queries per workgroup: four waves of 16
constexpr int H256_MIN_QUERIES = 4;  // fewer stay on k_attention, as for the other MFMA kinds
// [2 buffers] K block [32][256 + 8] halfs (33 16-byte chunks a row: odd, h16_krow's argument), then [2 buffers] V block transposed
// [256][32 + 8] halfs: 74 752 bytes -- past the 48 KiB a kernel gets unasked, two workgroups fit a CU's 160 KiB
constexpr int H256_LDS = 2 * H16_KB * h16_krow(H256_HD) * 2 + 2 * H256_HD * H16_VROW * 2;

enum AttnHeads256Error {             // 0 .. 5: AttnPlanError of plan_attention on the same facts
    ATTN256_ERR_HEAD_SIZE = 6,       // head_dim is not 256
    ATTN256_ERR_FEW_QUERIES = 7,     // q_tokens < 4
    ATTN256_ERR_ROWS_MODE = 8,       // ifa_attention_rows stays on k_attention
};
// The order of the fields is the order of ifa_attention_heads256_plan's `out` array.
struct AttnHeads256Plan {
    int error = ATTN_OK;
    int q_per_wg = 0;
    int grid_x = 0, grid_y = 0;      // (query tiles, heads)
    int lds = 0;                     // dynamic LDS bytes
    int xcd_remap = 0;               // the kernel maps (tile, head) so that an XCD keeps an eighth of the heads
};
constexpr int ATTN256_N_OUT = sizeof(AttnHeads256Plan) / sizeof(int);    // 6

inline AttnHeads256Plan plan_attention_heads256(const AttnFacts &f)
{
    AttnHeads256Plan r;
    auto refuse = [&](int e) { r = AttnHeads256Plan(); r.error = e; return r; };
    if (f.rows_mode) return refuse(ATTN256_ERR_ROWS_MODE);
    const AttnPlan base = plan_attention(f);             // dtype, heads, the cache row of whole 32-blocks, shape, length
    if (base.error != ATTN_OK) return refuse(base.error);
    if (f.head_dim != H256_HD) return refuse(ATTN256_ERR_HEAD_SIZE);
    if (f.q_tokens < H256_MIN_QUERIES) return refuse(ATTN256_ERR_FEW_QUERIES);
    r.q_per_wg = H256_QT;
    r.grid_x = (f.q_tokens + H256_QT - 1) / H256_QT;
    r.grid_y = f.heads;
    r.lds = H256_LDS;
    r.xcd_remap = f.heads % 8 == 0;
    return r;
}

} // namespace ifa
