// ifa_attn_heads.hip -- prompt attention on the matrix cores for head_dim 48 / 80 / 96 (Phi-2 / StableLM, Phi-3-mini geometries), and for
// 256 (Gemma) behind a plan of its own (launch_attention_heads256 at the end of the file).
//
// The 32 x 32 tile kernels of ifa_attn.hip need head_dim in multiples of 32 (the P.V output width) and have LDS swizzles written for 64
// and 128; these head sizes therefore ran k_attention: one workgroup per (head, query), scalar dots, the whole prefix re-read per query.
// k_attention_heads16 is built on 16 x 16 MFMA tiles, which divide all three sizes with no padding of the head:
//
//   split    one workgroup per (64-query tile, head); wave w owns queries 16 w .. 16 w + 15.  Waves of a last tile that hold no query
//            still stage and meet the barriers.  Grid (ceil(q_tokens / 64), heads), XCD remap as the other MFMA kinds.
//   Q        the wave's [16 x HD] block, loaded ONCE into registers as MFMA fragments (HD / 4 halfs per lane), kept for both passes.
//   K / V    32-key blocks through LDS, shared by the four waves, two buffers: block kb + 1 is stored and block kb + 2 requested from
//            global memory before block kb's MFMAs, one barrier per block.  K row-wise with one 16-byte chunk of pad (h16_krow: odd
//            chunk count, conflict-free fragment reads); V transposed [HD][32 + 8] with its key columns in the order of the
//            probabilities' registers (h16_col).  Q8_B32T2 rows are dequantised while staged, the scale taken by the ABSOLUTE column
//            (kv_head * HD + d) / 32 of the cache row: at 48 and 80 a 32-value block straddles two heads.
//   scores   S^T = K . Q^T, not Q . K^T: the keys are the MFMA rows and a query is a column, so a lane holds 8 keys (4 g + r and
//            16 + 4 g + r) of ONE query.  Masking, maximum, sum and the probabilities are then per-lane work; the four lanes of a query
//            meet once, at the end of pass 1 (two xor shuffles).  Per 16-key tile: HD / 32 steps of v_mfma_f32_16x16x32_f16 and, at 48
//            and 80, one v_mfma_f32_16x16x16_f16 tail (2 / 3 / 3 instructions against 3 / 5 / 6 of the x16 form, and b128 LDS reads).
//   P        from the score layout to the MFMA operand through registers, with NO cross-lane movement: O^T = V^T . P^T takes P^T as
//            the B operand -- lane = query column, 8 keys per lane -- which is what a lane already holds once V's key columns are stored
//            in that order.  A per-wave LDS patch (needed for Q . K^T, where a lane holds 4 queries of one key) would cost a store, a
//            wait and a load per block.
//   P . V    one v_mfma_f32_16x16x32_f16 per 16 output columns and 32-key block: HD / 16 = 3 / 5 / 6 accumulator tiles per wave.
//   passes   pass 1: every query's maximum and sum over its keys; pass 2: the scores again, P, P . V.  No score tile in LDS, no global
//            workspace, no host synchronisation: enqueue-only.  The rounding points are those of k_attention_2pass and of the oracle:
//            S = half(alpha * q.k) (+ ALiBi, rounded again), maximum / sum fp32, e = half(exp), P = half(e * 1 / sum), fp32
//            accumulation, out = half.
//   causal   a workgroup stops at the last key its last query sees; a wave skips the MFMAs (not the barriers) of blocks past its own 16
//            queries' edge; inside the diagonal blocks the mask is per element.
#include <cstring>
#include "ifa_host.h"
#include "ifa_device.h"
#include "ifa_math.h"
#include "ifa_attn_heads_plan.h"
#include "ifa_attn_heads256_plan.h"

namespace ifa {

typedef _Float16 h16_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16_half4 __attribute__((ext_vector_type(4)));
typedef float h16_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t h16_u32x4 __attribute__((ext_vector_type(4)));

// column of key k (0 .. 31) in the staged V block: lane group g = 0 .. 3 holds the probabilities of keys 4 g + r (first 16-key tile)
// and 16 + 4 g + r (second), and reads the 8 columns 8 g .. 8 g + 7 as its P.V operand
__host__ __device__ constexpr int h16_col(int k) { return 8 * ((k >> 2) & 3) + 4 * (k >> 4) + (k & 3); }

// 8 consecutive elements e0 .. e0 + 7 (e0 % 8 == 0, an ABSOLUTE column of the cache row) of kv-row j as halfs
template <bool Q8>
__device__ __forceinline__ h16_half8 h16_load8(const uint8_t *cache, size_t row_bytes, int j, int e0)
{
    if constexpr (Q8) {
        const uint8_t *blk = cache + (size_t)j * row_bytes + (size_t)(e0 >> 5) * 34;      // the 32-block of the column, whichever head it began in
        const uint16_t *p16 = reinterpret_cast<const uint16_t *>(blk);
        const float scale = hbits2f(p16[0]);
        h16_half8 r;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t two = p16[1 + ((e0 & 31) >> 1) + w];
            r[2 * w] = f2h((float)(int)(int8_t)(two & 0xFF) * scale);
            r[2 * w + 1] = f2h((float)(int)(int8_t)(two >> 8) * scale);
        }
        return r;
    } else {
        return __builtin_bit_cast(h16_half8, *reinterpret_cast<const h16_u32x4 *>(cache + (size_t)j * row_bytes + (size_t)e0 * 2));
    }
}

template <int HD, bool Q8>
__global__ void __launch_bounds__(256, 2) k_attention_heads16(const half_t *__restrict__ q, const uint8_t *__restrict__ kc,
                                                              const uint8_t *__restrict__ vc, int n_ctx, int q_tokens,
                                                              int prefix_len, int heads, int kv_heads, float kq_scale,
                                                              int alibi, int alibi_base, int alibi_total, half_t *__restrict__ out)
{
    static_assert(attn_heads16_head(HD) || HD == H256_HD, "16-wide tiles: head_dim 48 / 80 / 96, and 256 behind its own plan");
    constexpr int KS32 = HD / 32;                    // x32 reduction steps of a score tile
    constexpr bool TAIL = HD % 32 != 0;              // ... and one x16 step over the last 16 dims
    constexpr int NT = HD / 16;                      // 16-wide output tiles
    constexpr int CHK = HD / 8;                      // 16-byte chunks per K / V row of the head
    constexpr int NCH = 32 * CHK;                    // chunks of a 32-key block
    constexpr int NIT = (NCH + 255) / 256;           // ... per thread (48: 192 chunks, threads 192 .. 255 stage nothing)
    constexpr int KROW = h16_krow(HD);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t *const Ks = reinterpret_cast<half_t *>(smem);                           // [2][32][KROW]
    half_t *const Vs = Ks + 2 * H16_KB * KROW;                                     // [2][HD][H16_VROW]
    int tile = blockIdx.x, h = blockIdx.y;
    if (heads % 8 == 0) {            // an XCD keeps a fixed eighth of the heads (their K / V in ONE L2); longest tiles first
        const int w = blockIdx.y * gridDim.x + blockIdx.x, xcd = w & 7, r = w >> 3;
        h = (r / (int)gridDim.x) * 8 + xcd;
        tile = (int)gridDim.x - 1 - r % (int)gridDim.x;
    }
    const int t0 = tile * H16_QT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int kvh = h / (heads / kv_heads);
    const int kv_dim = kv_heads * HD;
    const size_t row_bytes = Q8 ? (size_t)(kv_dim / 32) * 34 : (size_t)kv_dim * 2;
    const int hoff = kvh * HD;
    const int n_keys = min(n_ctx, prefix_len + min(t0 + H16_QT, q_tokens));       // causal bound of the whole tile
    const int nkb = (n_keys + 31) / 32;
    const int tw = t0 + 16 * wave, tq = tw + i;
    const int n_valid = tq < q_tokens ? min(n_ctx, prefix_len + tq + 1) : 0;      // keys this lane's query may see
    const int wave_keys = tw < q_tokens ? min(n_ctx, prefix_len + min(tw + 16, q_tokens)) : 0;
    const int wave_nkb = (wave_keys + 31) / 32;                                   // blocks past it are fully masked for this wave
    const int full_keys = tw < q_tokens ? min(n_ctx, prefix_len + tw + 1) : 0;    // every query of the wave sees the keys below this
    const float alpha = 1.0f / sqrtf((float)HD) / kq_scale;
    const float mk = alibi ? alibi_slope(h + alibi_base, alibi_total) : 0.0f;

    // ---- Q fragments: lane (i, g) holds dims 32 s + 8 g .. + 7 of query tw + i per x32 step, dims HD - 16 + 4 g .. + 3 for the tail
    h16_half8 qf[KS32];
    h16_half4 qt4;
    {
        const half_t *qrow = q + ((size_t)min(tq, q_tokens - 1) * heads + h) * HD;
#pragma unroll
        for (int s2 = 0; s2 < KS32; s2++) qf[s2] = __builtin_bit_cast(h16_half8, *reinterpret_cast<const h16_u32x4 *>(qrow + 32 * s2 + 8 * g));
        if constexpr (TAIL) qt4 = *reinterpret_cast<const h16_half4 *>(qrow + HD - 16 + 4 * g);
    }
    // ---- staging.  K: chunk idx -> (row idx / CHK, chunk idx % CHK), rows as they are.  V: idx -> (key idx % 32, chunk idx / 32):
    // lane pairs hold an even and an odd key of the same 8 dims and trade halves, so that every lane stores (even key, odd key)
    // dwords of 4 dims -- half the LDS stores of a 2-byte transpose; a wave's 32 keys x 2 parities spread over all 32 banks
    h16_half8 kreg[NIT], vreg[NIT];
    auto kload = [&](int kb) {
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = min(tid + it * 256, NCH - 1), row = idx / CHK, c = idx % CHK;
            kreg[it] = h16_load8<Q8>(kc, row_bytes, min(32 * kb + row, n_ctx - 1), hoff + 8 * c);
        }
    };
    auto kstage = [&](int buf) {
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = tid + it * 256, row = idx / CHK, c = idx % CHK;
            if (idx < NCH) *reinterpret_cast<h16_half8 *>(Ks + ((size_t)buf * H16_KB + row) * KROW + 8 * c) = kreg[it];
        }
    };
    const int vpar = tid & 1;
    auto vload = [&](int kb) {
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = tid + it * 256, key = idx & 31, c = idx < NCH ? idx >> 5 : 0;
            vreg[it] = h16_load8<Q8>(vc, row_bytes, min(32 * kb + key, n_ctx - 1), hoff + 8 * c);
        }
    };
    auto swap1 = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false); };   // lane ^ 1 (quad_perm [1, 0, 3, 2])
    auto vstage = [&](int buf) {
        half_t *Vt = Vs + (size_t)buf * HD * H16_VROW;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = tid + it * 256, key = idx & 30, c = idx >> 5;            // (key: the even one of the pair)
            const h16_u32x4 w = __builtin_bit_cast(h16_u32x4, vreg[it]);
            const uint32_t m0 = vpar ? w[2] : w[0], m1 = vpar ? w[3] : w[1];         // the 4 dims this lane stores
            const uint32_t r0 = swap1(vpar ? w[0] : w[2]), r1 = swap1(vpar ? w[1] : w[3]);
            const uint32_t e0 = vpar ? r0 : m0, e1 = vpar ? r1 : m1;                 // even key's values
            const uint32_t o0 = vpar ? m0 : r0, o1 = vpar ? m1 : r1;                 // odd key's values
            if (idx < NCH) {
                uint32_t *dst = reinterpret_cast<uint32_t *>(Vt + (size_t)(8 * c + 4 * vpar) * H16_VROW + h16_col(key));
                dst[0 * H16_VROW / 2] = (e0 & 0xFFFFu) | (o0 << 16);
                dst[1 * H16_VROW / 2] = (e0 >> 16) | (o0 & 0xFFFF0000u);
                dst[2 * H16_VROW / 2] = (e1 & 0xFFFFu) | (o1 << 16);
                dst[3 * H16_VROW / 2] = (e1 >> 16) | (o1 & 0xFFFF0000u);
            }
        }
    };
    // scores of key block kb for this lane's query: x[4 t + r] = half(alpha * q.k (+ ALiBi)) as float, key = 32 kb + 16 t + 4 g + r;
    // masked keys: -inf.  exp(kq_scale * x - max) is exp2(fma(log2(e) * kq_scale, x, c)) with c = -log2(e) * kq_scale * max.
    const float l2e_kq = 1.44269504088896341f * kq_scale;
    auto scores = [&](int kb, float (&x)[8]) {
        const half_t *Kb = Ks + (size_t)(kb & 1) * H16_KB * KROW;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const half_t *krow = Kb + (size_t)(16 * t + i) * KROW;
            h16_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s2 = 0; s2 < KS32; s2++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h16_half8 *>(krow + 32 * s2 + 8 * g), qf[s2], acc, 0, 0, 0);
            // the tail is a chain of its own, added by the VALU.  Not only for the overlap: with the x32 result as the x16 instruction's
            // addend (back to back, the same registers) the first two of the four result registers came out wrong on the MI355X
            if constexpr (TAIL) {
                const h16_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
                const h16_f32x4 tail = __builtin_amdgcn_mfma_f32_16x16x16f16(*reinterpret_cast<const h16_half4 *>(krow + HD - 16 + 4 * g), qt4, zero, 0, 0, 0);
                acc += tail;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                half_t sv = f2h(alpha * acc[r]);
                if (alibi) sv = f2h((float)(32 * kb + 16 * t + 4 * g + r) * mk + h2f(sv));
                x[4 * t + r] = h2f(sv);
            }
        }
        if (32 * kb + 32 > full_keys) {                   // (wave-uniform: only the blocks on the causal edge)
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (32 * kb + 16 * (e >> 2) + 4 * g + (e & 3) >= n_valid) x[e] = -INFINITY;
        }
    };
    auto exp2_fast = [](float v) { return __builtin_amdgcn_exp2f(v); };

    // ---- pass 1: running max / sum of every query over its keys (a quarter of them per lane)
    float m = -INFINITY, sum = 0.0f;
    kload(0);
    kstage(0);
    kload(min(1, nkb - 1));
    __syncthreads();
    for (int kb = 0; kb < nkb; kb++) {
        kstage((kb + 1) & 1);                // (block kb + 1, or a harmless repeat of the last one)
        kload(min(kb + 2, nkb - 1));
        if (kb < wave_nkb) {
            float x[8];
            scores(kb, x);
            float bm = x[0];
#pragma unroll
            for (int e = 1; e < 8; e++) bm = fmaxf(bm, x[e]);
            if (bm > m) { sum *= exp2_fast(l2e_kq * (m - bm)); m = bm; }             // (m = -inf: sum is 0 and stays 0)
            if (m > -INFINITY) {
                const float c = -l2e_kq * m;
#pragma unroll
                for (int e = 0; e < 8; e++) sum += exp2_fast(__builtin_fmaf(l2e_kq, x[e], c));    // masked: 2^-inf = 0
            }
        }
        __syncthreads();
    }
    // the four lanes (g) of a query meet: lanes ^ 16, then ^ 32
    float M = m, tot = sum;
#pragma unroll
    for (int d = 16; d <= 32; d *= 2) {
        const float m2 = __shfl_xor(M, d), s2v = __shfl_xor(tot, d);
        const float Mn = fmaxf(M, m2);
        tot = (M > -INFINITY ? tot * exp2_fast(l2e_kq * (M - Mn)) : 0.0f) + (m2 > -INFINITY ? s2v * exp2_fast(l2e_kq * (m2 - Mn)) : 0.0f);
        M = Mn;
    }
    const float inv = tot > 0.0f ? 1.0f / tot : 0.0f;             // (rows past q_tokens: all zero)
    // ---- pass 2: P = half(half(exp(x - M)) / sum) from recomputed scores, O^T += V^T . P^T
    h16_f32x4 oacc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) oacc[nt] = h16_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    kload(0);
    vload(0);
    kstage(0);
    vstage(0);
    kload(min(1, nkb - 1));
    vload(min(1, nkb - 1));
    __syncthreads();
    for (int kb = 0; kb < nkb; kb++) {
        kstage((kb + 1) & 1);
        vstage((kb + 1) & 1);
        kload(min(kb + 2, nkb - 1));
        vload(min(kb + 2, nkb - 1));
        if (kb < wave_nkb) {
            const half_t *Vt = Vs + (size_t)(kb & 1) * HD * H16_VROW;
            float x[8];
            scores(kb, x);
            h16_half8 pb;                    // keys 4 g + r | 16 + 4 g + r: columns 8 g .. 8 g + 7 of the staged V block (h16_col)
            const float c = M > -INFINITY ? -l2e_kq * M : 0.0f;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const half_t ev = f2h(exp2_fast(__builtin_fmaf(l2e_kq, x[e], c)));      // masked keys: 2^-inf = 0
                pb[e] = f2h(h2f(ev) * inv);
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const h16_half8 vf = *reinterpret_cast<const h16_half8 *>(Vt + (size_t)(16 * nt + i) * H16_VROW + 8 * g);
                oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb, oacc[nt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // lane (i, g) holds dims 16 nt + 4 g .. + 3 of query tw + i
    if (tq < q_tokens) {
        half_t *orow = out + ((size_t)tq * heads + h) * HD;
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            h16_half4 o4;
#pragma unroll
            for (int e = 0; e < 4; e++) o4[e] = f2h(oacc[nt][e]);
            *reinterpret_cast<h16_half4 *>(orow + 16 * nt + 4 * g) = o4;
        }
    }
}

// ifa_attention's route to the kernel (ifa_attn.hip: with ifa_attention_mfma_heads(1), head_dim 48 / 80 / 96, q_tokens >= 4)
int launch_attention_heads16(const AttnHeads16Plan &pl, const void *q, const void *kcache, const void *vcache, int kv_dtype, int n_ctx,
                             int q_tokens, int prefix_len, int heads, int kv_heads, int head_dim, float kq_scale, int alibi,
                             int alibi_base, int alibi_total, void *out, hipStream_t s)
{
    IFA_REQUIRE(pl.error == ATTN_OK && pl.lds == attn_heads16_lds(head_dim), "ifa_attention: no plan for the 16-wide tile kernel (head_dim %d)", head_dim);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
#define IFA_H16(HDV, Q8V) k_attention_heads16<HDV, Q8V><<<grid, dim3(256), (size_t)pl.lds, s>>>((const half_t *)q, (const uint8_t *)kcache, (const uint8_t *)vcache, \
        n_ctx, q_tokens, prefix_len, heads, kv_heads, kq_scale, alibi, alibi_base, alibi_total, (half_t *)out)
    const bool q8 = kv_dtype == Q8_B32T2;
    switch (head_dim) {
    case 48: if (q8) IFA_H16(48, true); else IFA_H16(48, false); break;
    case 80: if (q8) IFA_H16(80, true); else IFA_H16(80, false); break;
    default: if (q8) IFA_H16(96, true); else IFA_H16(96, false); break;
    }
#undef IFA_H16
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// head_dim 256 (Gemma: 8 heads over 1 kv head, 16 over 16) behind plan_attention_heads256 (ifa_attn_heads256_plan.h): the same template.
// At 256 it is 8 x32 steps per score tile and no x16 tail, 16 output tiles (64 accumulator registers), 64 halfs of Q per lane (32
// registers), four staged chunks of K and of V per thread and block, a 32-value Q8 block inside one head; 182 (F16) / 222 (Q8)
// VGPRs, no scratch, two workgroups per CU.  Its 74 752 bytes of LDS are past what a kernel gets unasked, hence the attribute.
// A kernel written for this head size alone -- 128 queries per workgroup, a wave per 32 queries on v_mfma_f32_32x32x16_f16, Q (64
// registers) and eight 32 x 32 output tiles (128) in registers, one wave per SIMD, half the LDS operand bytes per flop -- was measured
// against this instantiation and lost at every size from 64 to 8192 queries (2048 queries, 16 heads, F16: 217 against 174 us): with one
// wave per SIMD nothing overlaps its LDS reads, its dependent 16-step MFMA chain and its softmax, and at 8 or 16 heads a prompt of 2048
// tokens gives 128-query tiles no more than one workgroup per CU.  docs/prompt_attention_heads256.md has the table.
int launch_attention_heads256(const AttnHeads256Plan &pl, const void *q, const void *kcache, const void *vcache, int kv_dtype, int n_ctx,
                              int q_tokens, int prefix_len, int heads, int kv_heads, float kq_scale, int alibi, int alibi_base,
                              int alibi_total, void *out, hipStream_t s)
{
    IFA_REQUIRE(pl.error == ATTN_OK && pl.lds == H256_LDS && pl.q_per_wg == H16_QT, "ifa_attention: no plan for 256-wide heads (error %d)", pl.error);
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
#define IFA_H256(Q8V) { auto kern = k_attention_heads16<H256_HD, Q8V>; \
        IFA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds)); \
        kern<<<grid, dim3(256), (size_t)pl.lds, s>>>((const half_t *)q, (const uint8_t *)kcache, (const uint8_t *)vcache, n_ctx, q_tokens, \
                                                     prefix_len, heads, kv_heads, kq_scale, alibi, alibi_base, alibi_total, (half_t *)out); }
    if (kv_dtype == Q8_B32T2) IFA_H256(true) else IFA_H256(false)
#undef IFA_H256
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifa

using namespace ifa;

// the launch plan of the kernel (ifa_attn_heads_plan.h) behind the C ABI, for tests: the pure function, no device is touched
extern "C" int ifa_attention_heads16_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == ATTN_N_FACTS && n_out >= ATTN16_N_OUT, "ifa_attention_heads16_plan: %d facts, %d outputs expected", ATTN_N_FACTS, ATTN16_N_OUT);
    AttnFacts f;
    memcpy(&f, facts, sizeof(f));
    const AttnHeads16Plan r = plan_attention_heads16(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}
