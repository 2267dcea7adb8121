// ifa_decode_draft_kv.hip -- the draft step (ifa_model_decode_draft): n rows of ONE query in one batched step, row i the token at
// position pos0 + i behind cache rows [0, pos0 + i).  Row 0 is the query's last committed token, rows 1 .. n - 1 are guessed
// continuations (lookup decoding, host/lookup_draft.h); the caller compares the step's greedy ids with its guesses and keeps the
// rows that turned out right.
//
// The batched step's attention kernel (k_dec_attn<.., BATCH>) rotates, stores and attends in one workgroup per (head, row): with
// two rows on the same slot a workgroup would read cache rows a sibling is still writing.  Here the K / V rows of ALL n rows go to
// the cache first, in one launch behind the wq | wk | wv product (k_draft_kv_store), and the attention kernel runs with
// DecAttnParams::skip_store: row i then finds rows pos0 .. pos0 + i - 1 in the cache like any other history row -- in the 256-row
// entry prefetch and in the loops past it -- and takes its own row from LDS as it always does.  Everything else is forward_batch.
//
// The arithmetic is the attention kernel's, expression for expression: the pair rotation is rope_apply on the row staged in LDS
// with the (cos, sin) pairs of m->brope (k_dec_batch_gather, one set per row), the F16 row is the rotated halves, the Q8_B32T2 row
// is the in-kernel store's quantiser (block maximum over 32 lanes, scale = max / 127, codes roundf(value / scale) clamped).  So the
// bytes equal what k_dec_attn<.., BATCH> writes for a query at that position, and row i of the step is bit for bit the row
// ifa_model_decode_batch computes for a query whose slot holds the same bytes in rows [0, pos0 + i).
#include "ifa_engine_state.h"

namespace ifae {

// grid (kv_heads, rows), 256 threads: one workgroup stages, rotates and stores the K and V slices of one kv head of one row.
// F16 cache: 16-byte vector stores (HD / 8 lanes per slice).  Q8 cache: one 32-value block per half wave, as in the attention kernel.
template <int HD, bool Q8>
__global__ void __launch_bounds__(256) k_draft_kv_store(const half_t *__restrict__ k, const half_t *__restrict__ v, int stride, int kv_heads,
                                                        const float *__restrict__ rope_tab, int rope_order, int rope_cols,
                                                        const AttnRowH *__restrict__ rows)
{
    static_assert(HD % 8 == 0 && HD <= 128 && (!Q8 || HD % 32 == 0), "head size: multiples of 8 up to 128 (Q8 rows: whole 32-blocks)");
    __shared__ __attribute__((aligned(16))) half_t kn[HD];
    __shared__ __attribute__((aligned(16))) half_t vn[HD];
    const int kvh = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AttnRowH br = rows[r];
    const int pos = br.n_ctx - 1;
    const int kv_dim = kv_heads * HD;
    const size_t row_bytes = Q8 ? (size_t)(kv_dim / 32) * 34 : (size_t)kv_dim * 2;
    const size_t head_off = Q8 ? (size_t)((kvh * HD) / 32) * 34 : (size_t)kvh * HD * 2;
    uint8_t *const kdst = (uint8_t *)br.kc + (size_t)pos * row_bytes + head_off;
    uint8_t *const vdst = (uint8_t *)br.vc + (size_t)pos * row_bytes + head_off;
    if (tid < HD) {
        kn[tid] = k[(size_t)r * stride + (size_t)kvh * HD + tid];
        vn[tid] = v[(size_t)r * stride + (size_t)kvh * HD + tid];
    }
    __syncthreads();
    if (rope_order != 0) {      // (uniform) the row's own (cos, sin) pairs: its position is pos0 + r
        if (tid < HD / 2) {
            const float *rt = rope_tab + (size_t)r * HD + 2 * tid;
            rope_apply(kn, tid, rt[0], rt[1], rope_order, rope_cols);
        }
        __syncthreads();
    }
    if constexpr (Q8) {
        constexpr int NB = HD / 32;
        for (int b = wave * 2 + (lane >> 5); b < 2 * NB; b += 8) {
            const half_t *src = b < NB ? kn : vn;
            const int bb = b < NB ? b : b - NB;
            const int l32 = lane & 31;
            const float val = h2f(src[bb * 32 + l32]);
            const float mx = half_wave_max(fabsf(val));
            const float sc = mx / 127;
            int qv = sc <= 0.000001f ? 0 : (int)roundf(val / sc);
            qv = min(max(qv, -128), 127);
            const half_t sch = f2h(sc);
            uint8_t *blk = (b < NB ? kdst : vdst) + (size_t)bb * 34;
            blk[2 + l32] = (uint8_t)(int8_t)qv;
            if (l32 == 0) *reinterpret_cast<uint16_t *>(blk) = __builtin_bit_cast(uint16_t, sch);
        }
    } else {
        // (a head's slice starts at a multiple of HD halves in a row of kv_dim halves, kv_dim % 8 == 0: every piece is 16-byte aligned)
        constexpr int DG = HD / 8;
        if (tid < DG) reinterpret_cast<u32x4 *>(kdst)[tid] = reinterpret_cast<const u32x4 *>(kn)[tid];
        else if (tid < 2 * DG) reinterpret_cast<u32x4 *>(vdst)[tid - DG] = reinterpret_cast<const u32x4 *>(vn)[tid - DG];
    }
}

int draft_kv_store_launch(ifa_model *m, int n, const half_t *k, const half_t *v, int stride, const void *rows_l)
{
    const ifa_model_config &c = m->cfg;
    const bool q8 = c.kv_dtype == Q8_B32T2;
    const int rope_cols = (int)(c.head_dim * c.partial_rotary + 0.5f);
    if ((c.kv_heads * c.head_dim) % 8 != 0) return ifa_fail(IFA_ERR_ARG, "draft step: kv_heads * head_dim = %d is not a multiple of 8", c.kv_heads * c.head_dim);
    const dim3 grid((unsigned)c.kv_heads, (unsigned)n), block(256);
#define IFA_DKV(HDV, Q8V) k_draft_kv_store<HDV, Q8V><<<grid, block, 0, m->stream>>>(k, v, stride, c.kv_heads, c.rope_order ? m->brope : nullptr, \
                                                                                     c.rope_order, rope_cols, (const AttnRowH *)rows_l)
    switch (c.head_dim) {
    case 32: if (q8) IFA_DKV(32, true); else IFA_DKV(32, false); break;
    case 64: if (q8) IFA_DKV(64, true); else IFA_DKV(64, false); break;
    case 96: if (q8) IFA_DKV(96, true); else IFA_DKV(96, false); break;
    case 128: if (q8) IFA_DKV(128, true); else IFA_DKV(128, false); break;
    case 48: if (q8) return ifa_fail(IFA_ERR_ARG, "draft step: Q8 cache with head_dim 48"); IFA_DKV(48, false); break;
    case 80: if (q8) return ifa_fail(IFA_ERR_ARG, "draft step: Q8 cache with head_dim 80"); IFA_DKV(80, false); break;
    default: return ifa_fail(IFA_ERR_ARG, "draft step: head_dim %d", c.head_dim);
    }
#undef IFA_DKV
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifae

extern "C" int ifa_model_decode_draft(ifa_model *m, int n, const int *tokens_host, int pos0, int *next_tokens_host, void *logits_out_dev)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode_draft: model not finalized");
    IFA_REQUIRE(tokens_host, "ifa_model_decode_draft: null tokens");
    IFA_REQUIRE(n >= 2 && n <= 8, "ifa_model_decode_draft: %d rows (2..8: the committed token and 1..7 draft tokens)", n);
    IFA_REQUIRE(pos0 >= 0 && (long long)pos0 + n <= (long long)m->cfg.max_ctx, "ifa_model_decode_draft: rows %d..%d outside max_ctx %d", pos0,
                pos0 + n - 1, m->cfg.max_ctx);
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_draft: partitioned workers have no draft step");
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_draft: option exact_order steps one row at a time; take ifa_model_decode");
    if (m->opt_perf_stat) return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_draft: option perf_stat times the single-row step; take ifa_model_decode");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    int pos[8], slot[8];
    for (int i = 0; i < n; i++) { pos[i] = pos0 + i; slot[i] = m->cur_slot; }
    StepTail none; TailCursor cur;
    return forward_batch(m, n, tokens_host, pos, slot, next_tokens_host, logits_out_dev, none, cur, true);
}
