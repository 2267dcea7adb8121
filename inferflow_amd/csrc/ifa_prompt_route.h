// ifa_prompt_route.h -- which route a prompt (ifa_model_forward) and a batched step (ifa_model_decode_batch) take through the linears of a
// layer, from which copy of the weights and what has to be built first, as pure host functions: no HIP calls, nothing of ifa_model.
// The engine fills in the facts (prompt_route_ready / batch_route_ready, ifa_engine_forward.hip) and acts on the plan; the C ABI exposes
// both for tests (ifa_prompt_route_plan, ifa_batch_route_plan, ifa_model_prompt_route).  Rules P1 - P12 and B1 - B5 of DESIGN.md
// ("Prompt route plan").
#pragma once
#include <algorithm>
#include <cstring>

namespace ifa {

// What the decision reads.  The order of the fields is the order of ifa_prompt_route_plan's `facts` array.
struct PromptRouteFacts {
    int T = 0;                           // tokens of the call
    int exact_order = 0, perf_stat = 0, prefill_chunk = 1, prefill_mid = 1, prefill_mid_max = 768, prefill_big = 1, prefill_big_min = 47,      // the options
        prefill_res_mid = 2048, rows_mo = 1, gemm_rows = 1, batch_fused = 1, gemm_splitk = 1, rows_kparts = 1;
    int topo = 0;                        // a multi-GPU partition drives the call
    int experts = 0;
    int rows_layers = 0;                 // wiring and linears take the rows GEMM: 0 no, 1 from MO copies only (a 64-weight format), 2 from the tiled layout too
    int big_layers = 0;                  // wiring and linears take the large-tile GEMM
    int mid_shapes = 0;                  // every linear can have an MO copy k_gemm_mid reads (cols % 128 == 0, rows % 16 == 0)
};
enum PromptRouteKind { PROMPT_EXACT = 0, PROMPT_OP_BY_OP = 1, PROMPT_ROWS = 2, PROMPT_MID = 3, PROMPT_BIG = 4 };
enum GmKernel { GM_K_ROWS = 0, GM_K_MID = 1, GM_K_BIG = 2 };      // gemm_rows_mfma_launch, gemm_mid, gemm_big
enum GmSource { GM_W_TILED = 0, GM_W_MO = 1, GM_W_X32 = 2 };      // Tensor::tiled, ::mo, ::x32 (or ::data where the format needs no copy)
struct GmPlan { int kernel = 0, src = 0, mo = 0, no_waits = 0; };      // one product: the kernel, its weights, GmArgs::mo and ::no_waits

// What a prompt runs.  The order of the fields is the order of ifa_prompt_route_plan's `out` array.
struct PromptRoute {
    int kind = PROMPT_OP_BY_OP;
    int first_pass = 0;                  // 32: the prompt runs as two passes, each planned as a prompt of its own when it runs; the other fields describe the first
    int norm_fused = 0;                  // Rows: the RMS norms are the prologue of the launch that reads them
    int res_mid = 0;                     // Big: wo / w2 through k_gemm_mid
    GmPlan qkv, wo, w13, w2;             // Rows / Mid / Big: wq | wk | wv, wo + residual, w1 / w3 + GLU, w2 + residual
    int need_mo = 0, need_x32 = 0;       // what has to exist before the launches (need_mo 2: built after the x32 copies)
    bool operator==(const PromptRoute &o) const { return std::memcmp(this, &o, sizeof(o)) == 0; }      // (ints only, no padding)
};
constexpr int PROMPT_ROUTE_N_FACTS = sizeof(PromptRouteFacts) / sizeof(int), PROMPT_ROUTE_N_OUT = sizeof(PromptRoute) / sizeof(int);      // 19, 22

// P4 / B2: a step of n rows through the rows GEMM
inline bool rows_route_ok(int batch_fused, int gemm_rows, int rows_mo, int rows_layers, int topo, int n)
{
    return batch_fused && gemm_rows && n >= 2 && n <= (rows_mo ? 32 : 16) && !topo && rows_layers >= (rows_mo ? 1 : 2);
}
inline GmPlan rows_gm(int rows_mo, int rows_kparts) { return GmPlan{GM_K_ROWS, rows_mo ? GM_W_MO : GM_W_TILED, rows_mo ? 1 : 0, !rows_kparts}; }

// Rules P1 - P12 of DESIGN.md ("Prompt route plan").
inline PromptRoute plan_prompt_route(const PromptRouteFacts &f)
{
    PromptRoute r;
    if (f.exact_order) { r.kind = PROMPT_EXACT; return r; }      // P1
    const bool big_ok = f.prefill_big && !f.topo && f.big_layers;
    const bool mid_asked = f.prefill_mid && f.rows_mo && f.T > 32 && f.experts == 0 && big_ok;      // P2 (it builds the copies before it looks at the shapes)
    const bool mid_tried = mid_asked && f.T <= f.prefill_mid_max, mid = mid_tried && f.mid_shapes;
    if (f.prefill_chunk && !f.topo && f.T >= 34 && f.T <= 48 && f.experts == 0) {      // P3: asked whatever perf_stat says
        if (!mid && rows_route_ok(f.batch_fused, f.gemm_rows, f.rows_mo, f.rows_layers, f.topo, 32)) {
            PromptRouteFacts g = f;
            g.T = 32; g.prefill_chunk = 0;
            r = plan_prompt_route(g);
            r.first_pass = 32;
        }
        r.need_mo = mid_tried;      // (what the question itself builds; each pass builds what it needs when it runs)
        if (r.first_pass) return r;
    }
    if (f.topo || f.perf_stat) return r;      // P5: op by op
    if (mid_tried) r.need_mo = 1;
    if (mid) {      // P6
        r.kind = PROMPT_MID;
        r.qkv = r.wo = r.w13 = r.w2 = GmPlan{GM_K_MID, GM_W_MO, 1, !f.gemm_splitk};
    } else if (f.T > std::max(32, f.prefill_big_min) && big_ok) {      // P7 - P9
        r.kind = PROMPT_BIG; r.need_x32 = 1;
        r.qkv = r.wo = r.w13 = r.w2 = GmPlan{GM_K_BIG, GM_W_X32, 0, !f.gemm_splitk};
        if (f.T <= f.prefill_res_mid && mid_asked) {
            if (!r.need_mo) r.need_mo = 2;
            r.res_mid = f.mid_shapes;
        }
        if (r.res_mid) r.wo = r.w2 = GmPlan{GM_K_MID, GM_W_MO, 1, !f.rows_kparts};
    } else if (f.experts == 0 && f.T <= 32 && rows_route_ok(f.batch_fused, f.gemm_rows, f.rows_mo, f.rows_layers, f.topo, f.T)) {      // P10 - P12
        r.kind = PROMPT_ROWS; r.need_mo = 1;
        r.norm_fused = f.T <= 8 || (f.rows_mo && f.T <= 16);
        r.qkv = r.wo = r.w13 = r.w2 = rows_gm(f.rows_mo, f.rows_kparts);
    }
    return r;
}

// The batched step.  The order of the fields is the order of ifa_batch_route_plan's `facts` array.
struct BatchRouteFacts {
    int n = 0;                           // rows of the call
    int exact_order = 0;
    int may_chunk = 0;                   // the call may run as several steps (ifa_model_decode_batch; never a single step, a draft step or a partition's)
    int rows_mo = 1, gemm_rows = 1, batch_fused = 1, rows_kparts = 1, batch_graph = 0, graph = 1;      // the options
    int topo = 0;
    int rows_layers = 0;                 // as PromptRouteFacts
    int has_moe = 0;                     // a layer routes its FFN over experts
    int logits_out = 0;                  // the caller wants every logits row
};
enum BatchRouteKind { BATCH_EXACT = 0, BATCH_OP_BY_OP = 1, BATCH_FUSED = 2 };
struct BatchRoute {
    int kind = BATCH_OP_BY_OP;
    int chunk = 0;                       // > 0: the call runs as steps of at most this many rows, each planned on its own; the other fields describe the first
    int norm_fused = 0;
    int captured = 0;                    // the step is captured once per row count and replayed
    GmPlan gm;                           // Fused: every product of the layer
    int need_mo = 0;
    bool operator==(const BatchRoute &o) const { return std::memcmp(this, &o, sizeof(o)) == 0; }
};
constexpr int BATCH_ROUTE_N_FACTS = sizeof(BatchRouteFacts) / sizeof(int), BATCH_ROUTE_N_OUT = sizeof(BatchRoute) / sizeof(int);      // 13, 9

// Rules B1 - B5 of DESIGN.md ("Prompt route plan").
inline BatchRoute plan_batch_route(const BatchRouteFacts &f)
{
    BatchRoute r;
    if (f.exact_order) { r.kind = BATCH_EXACT; return r; }      // B1
    auto rows_ok = [&](int n) { return rows_route_ok(f.batch_fused, f.gemm_rows, f.rows_mo, f.rows_layers, f.topo, n); };
    int n = f.n;
    const int fused_max = rows_ok(32) ? 32 : 16;
    if (f.may_chunk && n > fused_max && rows_ok(16)) {      // B3: balanced chunks
        const int k = (n + fused_max - 1) / fused_max;
        n = r.chunk = (n + k - 1) / k;
    }
    if (rows_ok(n)) {      // B2, B4
        r.kind = BATCH_FUSED; r.need_mo = 1;
        r.norm_fused = n <= 8 || (f.rows_mo && n <= 16);
        r.gm = rows_gm(f.rows_mo, f.rows_kparts);
    }
    r.captured = (f.batch_graph || r.kind == BATCH_FUSED) && f.graph && (!f.has_moe || r.kind == BATCH_FUSED) && !f.logits_out && !f.topo;      // B5
    return r;
}

} // namespace ifa
