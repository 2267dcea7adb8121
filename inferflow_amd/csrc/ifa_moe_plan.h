// ifa_moe_plan.h -- what a mixture-of-experts layer runs over the T rows of a step (ifa_engine_moe.hip): host-routed or device-routed,
// which router, the sizes of the device-built lists, which launches take the experts with 1 / 2..8 / more rows, whether the singles fork
// to the side stream -- as a pure host function: no HIP call, no ifa_model.  The engine fills the facts (moe_facts), the launchers
// follow the plan and decide nothing themselves; the C ABI exposes it for tests (ifa_moe_plan, ifa_model_moe_plan).  Rules M1 - M10 of
// DESIGN.md ("MoE layer plan"); the measurements behind the numbers are with the launchers.
#pragma once

namespace ifa {

// What the decision reads.  The order of the fields is the order of ifa_moe_plan's `facts` array.
struct MoeFacts {
    int T = 0;                           // rows of the step
    int experts = 0, top_k = 0, dim = 0;
    int ffn = 0;                         // rows of an expert's W1
    int w_dtype = -1;                    // the experts' format (for the record: the rules read it through w_ax8 / w_q4)
    int w_ax8 = 0;                       // ax8_eligible: the int8-activation GEMV reads it
    int w_q4 = 0;                        // Q4_B32T1A / B
    int full_quant_gemv = 0, norm_kind = 0;
    int gate_f16 = 0, gate_cols_match = 0;      // the router's weights: F16, dim columns
    int has_ffn_norm = 0;
    int experts_uniform = 0;             // all experts x 3 matrices present, per kind of one dtype / shape
    int have_table = 0, have_table_aos = 0, have_table_mo = 0;      // the pointer tables the layer holds now: tiled, reference layout, MO copies
    int moe_device = 1, moe_router_fused = 1, moe_singles = 1, moe_overlap = 1, gemm_rows = 1, rows_mo = 1;      // the options
    // the launchers' own predicates, evaluated by the engine
    int rows_use_mfma = 0;               // gemm_rows_use_mfma()
    int rows_mfma_ok = 0;                // gemm_rows_mfma_ok of both shapes at 2 rows
    int rows_q4_ok = 0;                  // gemm_rows_q4_grouped_cap > 0 for both widths
    int singles_ok = 0;                  // dec_singles_supported for both products
    int caller_norm = 0;                 // the caller hands over the rows BEFORE the FFN norm and wants norm and residual done by the layer
};
enum MoeKind {
    MOE_HOST = 0,                        // lists built on the host, expert by expert; synchronises the stream
    MOE_DEVICE_GROUPED = 1,              // lists built on the device, grouped launches per product: tiles, singles, small groups
    MOE_DEVICE_SINGLES = 2,              // no tile possible: the singles as two launches of the decode GEMV's structure, the small groups as two
};
enum MoeRouter {
    MOE_ROUTER_OPS = 0,                  // norm / gate product / softmax / top-k as launches of their own
    MOE_ROUTER_FUSED = 1,                // k_dec_moe_router: one launch, a workgroup per row
};
// What the layer runs.  The order of the fields is the order of ifa_moe_plan's `out` array.  A host-routed layer has the fields from
// tile_rows on at 0: it builds no device lists.
struct MoePlan {
    int kind = MOE_HOST;
    int router = MOE_ROUTER_OPS;         // T = 1: the router launch of the fused decode step (the host-routed body reads the gate's probabilities itself)
    int device_ok = 0;                   // the layer can be device-routed (whatever T)
    int cap = 0;                         // (row, expert) pairs of the step
    int tile_rows = 0;                   // rows of an MFMA tile of the grouped GEMM
    int small_max = 0;                   // experts with 2..small_max rows are small groups (0: none)
    int max_tiles = 0, max_singles = 0, max_smalls = 0;      // the most entries the device-built lists can hold: the grids of their launches
    int rows_kernel = 0;                 // the small groups stream their tiled Q4 weights once
    int rows_mfma = 0;                   // ... on the matrix cores
    int smalls_mo = 0;                   // ... from the MO copies: w1 | w3 gated in one launch, w2 in one
    int side_stream = 0;                 // the singles' two launches fork to the side stream
    int host_sync = 1;                   // the layer synchronises the stream: it may not be captured
};
constexpr int MOE_N_FACTS = sizeof(MoeFacts) / sizeof(int), MOE_N_OUT = sizeof(MoePlan) / sizeof(int);      // 28, 14

inline MoePlan plan_moe_layer(const MoeFacts &f)
{
    MoePlan r;
    r.device_ok = f.moe_device && f.have_table_aos && f.experts_uniform && f.w_ax8 && f.full_quant_gemv && f.dim % 32 == 0 && f.ffn % 32 == 0;      // M1
    const bool device = f.T > 1 && r.device_ok;      // M2
    // M3: what k_dec_moe_router covers.  One row (M4): a missing FFN norm is fine, the kernel copies.  Rows of a batched step (M5): a
    // workgroup per row up to 32, and only where the caller left the norm to the layer.
    const bool common = f.moe_router_fused && f.norm_kind == 0 && f.gate_f16 && f.dim % 8 == 0 && f.dim <= 16384 && f.experts <= 64 && f.gate_cols_match;
    const bool fused = f.T <= 1 ? common : (common && device && f.T <= 32 && f.has_ffn_norm && f.caller_norm);
    r.router = fused ? MOE_ROUTER_FUSED : MOE_ROUTER_OPS;
    r.cap = f.T * f.top_k;
    if (!device) return r;
    r.host_sync = 0;
    // M6: rows per expert on average >= 96: 128-row tiles (each decoded weight block feeds four MFMA tiles); else 64-row split-K tiles
    const int E = f.experts;
    r.tile_rows = r.cap / (E > 1 ? E : 1) >= 96 ? 128 : 64;
    r.max_singles = E < r.cap ? E : r.cap;
    // M7: a handful of rows per expert: experts with 2..8 rows stream their tiled Q4 weights once instead of filling a 64-row tile with padding
    r.rows_mfma = f.rows_use_mfma && f.rows_mfma_ok;
    r.rows_kernel = f.w_q4 && f.gemm_rows && f.have_table && r.cap <= 8 * E && (r.rows_mfma || f.rows_q4_ok);
    r.small_max = r.rows_kernel ? 8 : 0;
    r.max_smalls = r.rows_kernel ? (E < r.cap / 2 ? E : r.cap / 2) : 0;
    r.smalls_mo = r.rows_mfma && f.rows_mo && f.have_table_mo && r.max_smalls > 0;
    // M8: T <= small_max: no expert can collect more rows than the small groups take -- the tile list stays empty
    r.max_tiles = (r.small_max > 0 && f.T <= r.small_max) ? 0 : r.cap / r.tile_rows + E;
    // M9: no tiles, and the small groups gate their own products (or there are none): the singles are the only rows the quantiser and
    // element-wise launches of the grouped route would serve
    const bool singles = f.moe_singles && r.max_tiles == 0 && (r.smalls_mo || r.max_smalls == 0) && f.have_table && f.singles_ok;
    r.kind = singles ? MOE_DEVICE_SINGLES : MOE_DEVICE_GROUPED;
    r.side_stream = singles && f.moe_overlap && r.max_smalls > 0;      // M10
    return r;
}

} // namespace ifa
