// ifa_decode_route.h -- which decode attention kernel instance a step runs, with which template arguments and how much LDS, as pure
// host functions: no HIP calls, nothing of ifa_model.  The engine fills in the facts (decode_route_ready, ifa_engine_decode.hip) and
// its launches act on the plan; the C ABI exposes both for tests (ifa_decode_route_plan, ifa_model_decode_route).  The LDS size
// formulas of the attention kernels live here too (constexpr: one definition for host and device, ifa_decode_attn.h).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

static constexpr size_t IFA_LDS_LIMIT = 160 * 1024;      // LDS per workgroup on gfx950 (MI355X_MICROARCH.md)

namespace ifa {
constexpr int DEC_ATTN_MAX_SPLITS = 32;      // splits per head of the keys-split-over-workgroups kernels (R7)
constexpr int DEC_PV_STAGE = 4096;           // keys of the score row k_dec_attn_pv stages per pass (multiple of 256)

// dynamic LDS bytes.  k_dec_attn_scores: staging of 256 F16 key rows (a Q8 cache is read straight into registers); k_dec_attn_pv: partial
// sums, the staged piece of the score row, this split's probabilities; k_dec_attn / the tail of k_dec_qkv_attn: q | k | v of the step,
// partial sums, the K tile (ktile_rows > 0), the score row [max_ctx]
constexpr size_t dec_attn_scores_smem(int head_dim, bool q8) { return q8 ? 16 : (size_t)256 * (head_dim * 2 + 16); }
constexpr size_t dec_attn_pv_smem(int head_dim, int max_ctx, int nsplits = 8)
{
    const size_t nsplit = 256 / (head_dim / 8);
    const size_t chunk = (((size_t)max_ctx + nsplits - 1) / nsplits + 63) / 64 * 64;
    return 8 * 4 + nsplit * head_dim * 4 + (size_t)(DEC_PV_STAGE + 8) * 2 + chunk * 2 + 16;
}
constexpr size_t dec_attn_smem(int head_dim, int max_ctx, int ktile_rows = 0)
{
    const size_t nsplit = 256 / (head_dim / 8);
    return (size_t)head_dim * 3 * 2 + 16 * 4 + nsplit * head_dim * 4 + (size_t)ktile_rows * head_dim * 2 + (((size_t)max_ctx * 2 + 15) & ~(size_t)15) + 16;
}

// the shapes of the fused QKV launch that have UL instances (the heads' workgroups take no weight rows): rw rows per wave over gk
// workgroups per kv group -- Llama-2-7B (6, 8) and Mixtral-8x7B (3, 32) on 256 CUs
inline bool dec_qkv_attn_ul_shape(int rw, int gk) { return (rw == 6 && gk == 8) || (rw == 3 && gk == 32); }

// What the decision reads.  The order of the fields is the order of ifa_decode_route_plan's `facts` array.
struct DecRouteFacts {
    int head_dim = 0, heads = 0, kv_heads = 0, max_ctx = 0, kv_q8 = 0;
    int reach = 0;                       // start_pos + n_steps of the call
    int attn_split_ctx = -1, attn_nsplits = 0, attn_kt = 1, attn_unload = 1, fuse_attn = 1, fuse_ffn = 0, attn_q8 = 1;      // the options
    int tail_layers_ok = 0, gk = 0, rw = 0;      // every layer can take the attention as the tail of its QKV launch, with this geometry
    int chain_level = 0;                 // what wiring and weights allow of the chained launch: 0, 1 (W1 | W3 -> W2), 2 (Wo -> ... too)
    int have_attq = 0;                   // the quantised image of the attention output exists
    int waits = 1;                       // launches whose workgroups wait for each other are allowed
    int num_cus = 0, visible_cus = 0;
    int own_launches = 0;                // the caller launches QKV, attention and FFN one by one (the tensor-parallel step): never FusedTail, no chain; R2 unchanged
};
enum DecRouteKind { DEC_ROUTE_ONE_WORKGROUP = 0, DEC_ROUTE_SPLIT = 1, DEC_ROUTE_FUSED_TAIL = 2 };

// What a step runs.  The order of the fields is the order of ifa_decode_route_plan's `out` array.
struct DecRoute {
    int kind = DEC_ROUTE_ONE_WORKGROUP;
    int nsplits = 0;                     // Split: splits per head
    int pb = 256, kt = 0, ul = 0;        // OneWorkgroup / FusedTail: the template arguments of the instance that is launched
    int gk = 0, rw = 0;                  // FusedTail: workgroups per kv group, rows per wave
    int chain = 0;                       // 0: single launches; 1: W1 | W3 -> W2 as one launch; 2: Wo -> W1 | W3 -> W2
    int split_threshold = 0, split = 0;  // R2, R3 (split 0 on a Split route: the LDS alone forced it)
    int lds_attn = 0;                    // dynamic LDS bytes: k_dec_attn, or the attention's part of k_dec_qkv_attn
    int lds_scores = 0, lds_pv = 0;      // k_dec_attn_scores, k_dec_attn_pv
    int error = 0;                       // 1: lds_pv exceeds the LDS (no launch)
    bool operator==(const DecRoute &o) const { return std::memcmp(this, &o, sizeof(o)) == 0; }      // (ints only, no padding)
};
constexpr int DEC_ROUTE_N_FACTS = sizeof(DecRouteFacts) / sizeof(int), DEC_ROUTE_N_OUT = sizeof(DecRoute) / sizeof(int);      // 22, 14

// Rules R1 - R10 of DESIGN.md ("Decode route plan").
inline DecRoute plan_decode_route(const DecRouteFacts &f)
{
    DecRoute r;
    const bool tail_possible = f.fuse_attn && f.waits && dec_attn_smem(f.head_dim, f.max_ctx, 256) <= IFA_LDS_LIMIT && f.tail_layers_ok && (long long)f.kv_heads * f.gk <= (long long)f.visible_cus;      // R1
    r.split_threshold = f.attn_split_ctx >= 0 ? f.attn_split_ctx : (tail_possible && f.attn_unload) ? (f.heads > f.kv_heads ? 640 : 512) : 320;      // R2
    r.split = (r.split_threshold > 0 && f.reach > r.split_threshold) ? (f.reach > 8192 ? 16 : 8) : 0;      // R3
    const int bucket = f.reach <= 64 ? 64 : (f.reach <= 128 ? 128 : 256);      // R4
    const bool lds_split = dec_attn_smem(f.head_dim, f.max_ctx, 0) > IFA_LDS_LIMIT;      // R5
    r.kind = (r.split || lds_split) ? DEC_ROUTE_SPLIT : (tail_possible && !f.own_launches) ? DEC_ROUTE_FUSED_TAIL : DEC_ROUTE_ONE_WORKGROUP;      // R6
    const bool kt_fits = f.attn_kt && !f.kv_q8 && dec_attn_smem(f.head_dim, f.max_ctx, bucket) <= IFA_LDS_LIMIT;
    if (r.kind == DEC_ROUTE_SPLIT) {      // R7
        r.pb = 0; r.nsplits = r.split > 1 ? r.split : 8;
        while (r.nsplits < DEC_ATTN_MAX_SPLITS && dec_attn_pv_smem(f.head_dim, f.max_ctx, r.nsplits) > IFA_LDS_LIMIT) r.nsplits *= 2;
        if (f.attn_nsplits > 0) r.nsplits = std::min(f.attn_nsplits, DEC_ATTN_MAX_SPLITS);
        r.lds_scores = (int)dec_attn_scores_smem(f.head_dim, f.kv_q8 != 0); r.lds_pv = (int)dec_attn_pv_smem(f.head_dim, f.max_ctx, r.nsplits);
        r.error = (size_t)r.lds_pv > IFA_LDS_LIMIT;
    } else if (r.kind == DEC_ROUTE_ONE_WORKGROUP) {      // R8
        const bool pow2 = f.head_dim == 32 || f.head_dim == 64 || f.head_dim == 128;      // (48, 80, 96: the 256-row instance only)
        r.pb = pow2 ? bucket : 256; r.kt = kt_fits && pow2;
    } else {      // R9
        r.kt = kt_fits;
        const bool unload = (f.attn_unload >= 1 && bucket == 256) || (f.attn_unload >= 2 && bucket == 128 && (r.kt || f.kv_q8));
        r.ul = unload && dec_qkv_attn_ul_shape(f.rw, f.gk);
        r.pb = (r.ul && bucket == 64) || (!f.kv_q8 && !r.kt) ? 256 : bucket;
        r.gk = f.gk; r.rw = f.rw;
    }
    if (r.kind != DEC_ROUTE_SPLIT) r.lds_attn = (int)dec_attn_smem(f.head_dim, f.max_ctx, r.kt ? r.pb : 0);
    if (!f.own_launches) {      // R10
        r.chain = (f.fuse_ffn && f.waits && f.num_cus <= f.visible_cus) ? std::min(f.fuse_ffn, 2) : 0;
        if (r.chain == 2 && (!f.have_attq || !f.attn_q8 || f.head_dim % 32 != 0)) r.chain = 1;
        r.chain = std::min(r.chain, f.chain_level);
    }
    return r;
}

} // namespace ifa
