// ifa_decode_attn256.h -- the decode attention for 256-wide heads (Gemma): batch-1 k_dec_attn256 (one workgroup per head) and
// k_dec_attn256_scores (keys split over workgroups; k_dec_attn_pv<256> / k_dec_attn_combine<256> finish that step), and
// k_dec_attn256_batch (the batched and the draft step: one workgroup per (head, row)).
//
// dec_attn_body gives every lane a whole key row in registers: at 256 that is 128 VGPRs of key per lane (and as many of q in
// k_dec_attn_scores).  Here a key row is split over a QUAD of lanes:
//   F16 cache   quad lane l holds the 16-byte pieces l, l + 4, ..., l + 28 of the row (dims 8 (l + 4 i) + e): every load instruction
//               of a quad is one contiguous 64-byte request, a wave instruction covers 16 rows
//   Q8 cache    a head's slice of a row is 8 blocks x 34 bytes; quad lane l holds blocks 2 l, 2 l + 1 (68 bytes at a 4-byte-aligned
//               offset, dims 64 l .. 64 l + 63) and dequantises them in registers, value = half(code x scale) as everywhere else
// A lane keeps only ITS 64 halves of the rotated q (32 VGPRs), adds its 64 products in fp32 in a fixed order, and the quad's four
// sums are added by two DPP quad permutes: (c_l + c_l^1) + (c_l^2 + c_l^3).  256 threads score 64 keys per pass; the rows of the next
// pass are requested before the products of the current one (64 VGPRs of keys in flight).  Lane 0 of the quad rounds alpha x sum
// (+ ALiBi) to F16 -- the rounding point of dec_attn_body.  Softmax and P.V keep that body's rounding points too (probabilities from
// F16 scores, fp32 sums; P.V with DG = 32 threads per V row, the 8 key residues mod 8 in parallel, partial sums through LDS).
// The sum of a key's products is NOT the reference's single chain in d order: the result is held to float64 within the bound of
// docs/decode_attention_edges.md, not to the oracle's bits (docs/decode_attention_heads256.md).
#pragma once
#include "ifa_decode_attn.h"

namespace ifa {

constexpr int D256 = 256;                          // the head size of this file
constexpr int D256_PASS = 64;                      // keys per pass of a 256-thread workgroup (a quad per key)
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
#ifndef IFA_GP      // (dec_attn_body's: cache rows through pointers whose address space is stated)
#define IFA_GP(T, p) ((const __attribute__((address_space(1))) T *)(p))
#endif

// a quad lane's share of one key row, as loaded
template <bool Q8>
struct Dec256Key {
    u32x4 w[Q8 ? 4 : 8];
    uint32_t t;                                    // Q8: bytes 64 .. 67 of the lane's 68
};

// head-relative start of quad lane l's share: rowp = cache + row * row_bytes + head_off
template <bool Q8>
__device__ __forceinline__ void dec256_load_key(Dec256Key<Q8> &K, const uint8_t *rowp, int l)
{
    if constexpr (!Q8) {
#pragma unroll
        for (int i = 0; i < 8; i++) K.w[i] = IFA_GP(u32x4, rowp)[l + 4 * i];
        K.t = 0;
    } else {
        const uint8_t *p = rowp + 68 * l;
#pragma unroll
        for (int i = 0; i < 4; i++) K.w[i] = *IFA_GP(u32x4_a4, p + 16 * i);
        K.t = *IFA_GP(uint32_t, p + 64);
    }
}

// the lane's 64 halves of a row staged in LDS (the rotated q, the new token's key), in the order of the lane's key dims
template <bool Q8>
__device__ __forceinline__ void dec256_lds_share(half8_t (&dst)[8], const half_t *row, int l)
{
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i] = *reinterpret_cast<const half8_t *>(row + (Q8 ? 64 * l + 8 * i : 8 * (l + 4 * i)));
}

// the lane's share of a cached row as halves: F16 bits as they are, Q8 blocks dequantised (half(code x scale), scale = the block's F16)
template <bool Q8>
__device__ __forceinline__ void dec256_key_halves(half8_t (&dst)[8], const Dec256Key<Q8> &K)
{
    if constexpr (!Q8) {
#pragma unroll
        for (int i = 0; i < 8; i++) dst[i] = __builtin_bit_cast(half8_t, K.w[i]);
    } else {
        // byte B (compile-time) of the 68; block b = bytes [34 b, 34 b + 34): scale, 32 codes
        auto kb = [&](int B) -> uint32_t { return ((B < 64 ? K.w[B >> 4][(B >> 2) & 3] : K.t) >> (8 * (B & 3))) & 0xFFu; };
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const float sc = hbits2f((uint16_t)(kb(34 * b) | (kb(34 * b + 1) << 8)));
#pragma unroll
            for (int i = 0; i < 32; i++)
                dst[(32 * b + i) >> 3][i & 7] = f2h((float)(int)(int8_t)kb(34 * b + 2 + i) * sc);
        }
    }
}

// the quad's dot product: every lane returns (c_l + c_l^1) + (c_l^2 + c_l^3), c = the lane's 64 products in one fp32 chain.  All four
// lanes of the quad must be active.
__device__ __forceinline__ float dec256_quad_dot(const half8_t (&q)[8], const half8_t (&k)[8])
{
    float c = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int e = 0; e < 8; e++) c = __builtin_fmaf((float)q[i][e], (float)k[i][e], c);
    }
    c = c + dpp_xor1(c);
    c = c + dpp_xor2(c);
    return c;
}

// The Q8 round trip of the new token's k and v rows (the expressions of dec_attn_body's store, one 32-value block per half wave: 8 + 8
// blocks on 8 half waves, two rounds): row p of both caches by the writer, the dequantised values back into kn / vn.
__device__ __forceinline__ void dec256_store_q8(half_t *kn, half_t *vn, uint8_t *kc, uint8_t *vc, size_t row_off, bool writer, int wave, int lane)
{
    constexpr int NB = D256 / 32;
    for (int b = wave * 2 + (lane >> 5); b < 2 * NB; b += 8) {
        half_t *src = b < NB ? kn : vn;
        const int bb = b < NB ? b : b - NB;
        const int l32 = lane & 31;
        const float val = h2f(src[bb * 32 + l32]);
        const float mx = half_wave_max(fabsf(val));
        const float sc = mx / 127;
        int qv = sc <= 0.000001f ? 0 : (int)roundf(val / sc);
        qv = min(max(qv, -128), 127);
        const half_t sch = f2h(sc);
        if (writer) {
            uint8_t *blk = (b < NB ? kc : vc) + row_off + (size_t)bb * 34;
            blk[2 + l32] = (uint8_t)(int8_t)qv;
            if (l32 == 0) *reinterpret_cast<uint16_t *>(blk) = __builtin_bit_cast(uint16_t, sch);
        }
        src[bb * 32 + l32] = f2h((float)qv * h2f(sch));   // dequantised value, as GetKRows returns it
    }
}

// stage the new token's q | k | v (one value per thread), rotate q (threads [0, 128)) and k ([128, 256)), store row p.  qs / kn / vn are
// final behind the last barrier in here (a Q8 cache: the one behind the round trip).
template <bool Q8>
__device__ __forceinline__ void dec256_stage_new(half_t *qs, half_t *kn, half_t *vn, half_t q_in, half_t k_in, half_t v_in, float rope_c, float rope_s,
                                                 const DecAttnParams &P, uint8_t *kc, uint8_t *vc, size_t row_off, bool store, bool writer)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    qs[tid] = q_in; kn[tid] = k_in; vn[tid] = v_in;
    __syncthreads();
    if (P.rope_order != 0) {
        rope_apply(tid < D256 / 2 ? qs : kn, tid < D256 / 2 ? tid : tid - D256 / 2, rope_c, rope_s, P.rope_order, P.rope_cols);
        __syncthreads();
    }
    if (!store) return;                 // (uniform: a split that does not own the new row)
    if constexpr (Q8) {
        dec256_store_q8(kn, vn, kc, vc, row_off, writer, wave, lane);
        __syncthreads();
    } else if (writer) {
        reinterpret_cast<half_t *>(kc + row_off)[tid] = kn[tid];
        reinterpret_cast<half_t *>(vc + row_off)[tid] = vn[tid];
    }
}

// What follows the scores of a whole row in LDS (S [n_ctx], every thread's lmax): softmax and P.V with dec_attn_body's rounding points;
// returns output element `tid` of the head in fp32.  Row n_ctx - 1 is the step's own: its value comes from vn (LDS), and no request
// goes past the last cached row n_ctx - 2.
template <bool Q8>
__device__ __forceinline__ float dec256_softmax_pv(half_t *S, float *red, float *opart, const half_t *vn, const uint8_t *pvc, size_t row_bytes,
                                                   size_t head_off, int n_ctx, float lmax, float kq_scale)
{
    constexpr int HD = D256, DG = HD / 8, NSPLIT = 256 / DG;       // 32 threads per V row, 8 key residues
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pos = n_ctx - 1, jlast = max(pos - 1, 0);
    // ---- softmax over S (probabilities from the F16 scores, fp32 sum, F16 e and P)
    lmax = wave_max(lmax);
    if (lane == 0) red[wave] = lmax;
    __syncthreads();
    const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float lsum = 0.0f;
    for (int j = tid; j < n_ctx; j += 256) {
        const float e = expf(kq_scale * h2f(S[j]) - mx);
        lsum += e;
        S[j] = f2h(e);
    }
    lsum = wave_sum(lsum);
    if (lane == 0) red[4 + wave] = lsum;
    __syncthreads();
    const float inv = 1.0f / (((red[4] + red[5]) + red[6]) + red[7]);
    for (int j = tid; j < n_ctx; j += 256) S[j] = f2h(h2f(S[j]) * inv);
    __syncthreads();

    // ---- O = P.V: thread (sp, dg) accumulates keys sp, sp + 8, ... for its 8 dims, groups of TB keys, the next group requested
    // before the current one is multiplied (clamped rows)
    const int dg = tid % DG, sp = tid / DG;
    constexpr int TB = 8;
    u32x4 vcur[Q8 ? 1 : TB], vnxt[Q8 ? 1 : TB];
    uint32_t sc_c[Q8 ? TB : 1], cw_c[Q8 ? TB : 1][2], sc_n[Q8 ? TB : 1], cw_n[Q8 ? TB : 1][2];      // Q8: block scale (half bits), the thread's 8 codes
    const size_t vq_off = head_off + (size_t)(dg / 4) * 34;
    auto vload = [&](u32x4 (&dst)[Q8 ? 1 : TB], uint32_t (&ds)[Q8 ? TB : 1], uint32_t (&dc)[Q8 ? TB : 1][2], int j0) {
#pragma unroll
        for (int u = 0; u < TB; u++) {
            const int jr = min(j0 + u * NSPLIT, jlast);
            if constexpr (!Q8) dst[u] = IFA_GP(u32x4, pvc + (size_t)jr * row_bytes + head_off)[dg];
            else {
                const auto *blk = IFA_GP(uint16_t, pvc + (size_t)jr * row_bytes + vq_off);
                typedef uint32_t u32x2_a2 __attribute__((ext_vector_type(2), aligned(2)));
                ds[u] = blk[0];
                const u32x2_a2 cw = *IFA_GP(u32x2_a2, blk + 1 + (dg % 4) * 4);
                dc[u][0] = cw[0]; dc[u][1] = cw[1];
            }
        }
    };
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = 0.0f;
    vload(vcur, sc_c, cw_c, sp);
    for (int j = sp; j < n_ctx; j += TB * NSPLIT) {
        vload(vnxt, sc_n, cw_n, j + TB * NSPLIT);
#pragma unroll
        for (int u = 0; u < TB; u++) {
            const int jj = j + u * NSPLIT;
            if (jj >= n_ctx) break;
            const float pj = h2f(S[jj]);
            half8_t v8;
            if (jj == pos) v8 = *reinterpret_cast<const half8_t *>(vn + dg * 8);
            else if constexpr (!Q8) v8 = __builtin_bit_cast(half8_t, vcur[u]);
            else {
                const float sc = hbits2f((uint16_t)sc_c[u]);
#pragma unroll
                for (int e = 0; e < 8; e++) v8[e] = f2h((float)(int)(int8_t)((cw_c[u][e >> 2] >> (8 * (e & 3))) & 0xFFu) * sc);
            }
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = __builtin_fmaf(pj, (float)v8[e], o[e]);
        }
#pragma unroll
        for (int u = 0; u < TB; u++) {
            if constexpr (Q8) { sc_c[u] = sc_n[u]; cw_c[u][0] = cw_n[u][0]; cw_c[u][1] = cw_n[u][1]; }
            else vcur[u] = vnxt[u];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) opart[sp * HD + dg * 8 + e] = o[e];
    __syncthreads();
    float acc = opart[tid];
    for (int s2 = 1; s2 < NSPLIT; s2++) acc = acc + opart[s2 * HD + tid];      // residue order
    return acc;
}

// One workgroup (256 threads) per query head: k_dec_attn<HD, Q8, false, 256, false>'s job at HD = 256.  Dynamic LDS:
// dec_attn_smem(256, max_ctx, 0) -- q | k | v, red[16], opart[8][256], the score row.  The leading scalar arguments are k_dec_attn's
// (preloaded into SGPRs): the first pass's rows (keys 0 .. 63: the cache holds at least DEC_ATTN_MIN_ROWS rows) are requested before
// the position is known.
template <bool Q8>
__global__ void __launch_bounds__(256) k_dec_attn256(const half_t *pq, const uint8_t *pkc, const uint8_t *pvc, int pheads, int pkvh, const DecAttnParams P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HD = D256, DG = HD / 8, NSPLIT = 256 / DG;       // 32 threads per V row, 8 key residues
    half_t *qs = reinterpret_cast<half_t *>(smem);
    half_t *kn = qs + HD;
    half_t *vn = kn + HD;
    float *red = reinterpret_cast<float *>(vn + HD);               // [16]
    float *opart = red + 16;                                       // [NSPLIT][HD]
    half_t *S = reinterpret_cast<half_t *>(opart + NSPLIT * HD);   // [n_ctx]
    const int h = blockIdx.x, tid = threadIdx.x;
    const int ql = tid & 3, qk = tid >> 2;                         // quad lane, key of the pass
    const int group = pheads / pkvh, kvh = h / group;
    const bool writer = (h % group) == 0;
    const size_t row_bytes = Q8 ? (size_t)pkvh * (HD / 32) * 34 : (size_t)pkvh * HD * 2;
    const size_t head_off = Q8 ? (size_t)kvh * (HD / 32) * 34 : (size_t)kvh * HD * 2;

    // ---- the new token's values and the (cos, sin) pair first, the first pass's rows behind them (all unconditional)
    const half_t q_in = pq[(size_t)h * HD + tid], k_in = pq[(size_t)(pheads + kvh) * HD + tid], v_in = pq[(size_t)(pheads + pkvh + kvh) * HD + tid];
    float rope_c = 1.0f, rope_s = 0.0f;
    {
        const int c = tid < HD / 2 ? tid : tid - HD / 2;
        const float *rt = P.rope_tab ? P.rope_tab : reinterpret_cast<const float *>(pq);      // (a valid dummy address without RoPE)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 cs = *IFA_GP(f32x2, rt + 2 * c);
        if (P.rope_order != 0) { rope_c = cs[0]; rope_s = cs[1]; }
    }
    Dec256Key<Q8> kcur, knxt;
    dec256_load_key<Q8>(kcur, pkc + (size_t)qk * row_bytes + head_off, ql);
    const int pos = *(const __attribute__((address_space(4))) int *)(P.state + 1);      // (scalar load: see dec_attn_body)
    const int n_ctx = pos + 1;
    dec256_stage_new<Q8>(qs, kn, vn, q_in, k_in, v_in, rope_c, rope_s, P, P.kcache, P.vcache, (size_t)pos * row_bytes + head_off, true, writer);

    // ---- scores: a quad per key, 64 keys per pass
    half8_t qreg[8];
    dec256_lds_share<Q8>(qreg, qs, ql);
    const float alpha = 1.0f / sqrtf((float)HD) / P.kq_scale;
    const float mk = P.alibi ? alibi_slope(h + P.alibi_base, P.alibi_total) : 0.0f;
    float lmax = -INFINITY;
    for (int jb = 0; jb < n_ctx; jb += D256_PASS) {
        const int j = jb + qk;
        // the next pass's rows (clamped to the last cached row: past the context nothing is used)
        dec256_load_key<Q8>(knxt, pkc + (size_t)min(j + D256_PASS, max(pos - 1, 0)) * row_bytes + head_off, ql);
        half8_t kh[8];
        if (j == pos) dec256_lds_share<Q8>(kh, kn, ql);       // the new token's (round-tripped) key never leaves the LDS
        else dec256_key_halves<Q8>(kh, kcur);
        const float c = dec256_quad_dot(qreg, kh);
        if (ql == 0 && j < n_ctx) {
            half_t s = f2h(alpha * c);
            if (P.alibi) { float a = (float)j * mk; s = f2h(a + h2f(s)); }
            S[j] = s;
            lmax = fmaxf(lmax, P.kq_scale * h2f(s));
        }
        kcur = knxt;
    }
    const float acc = dec256_softmax_pv<Q8>(S, red, opart, vn, pvc, row_bytes, head_off, n_ctx, lmax, P.kq_scale);
    const half_t yh = f2h(acc);
    P.out[(size_t)h * HD + tid] = yh;
    if (P.xq) dec_attn_emit_q8<HD>(P.xq, pheads * HD, h, tid, yh);
}

// The batched and the draft step, grid (heads, rows): k_dec_attn<HD, Q8, true>'s job at HD = 256, one workgroup per (head, row) with
// the quad mapping above.  Row b's cache pointers and context come from DecAttnBatchRow[b] (one scalar fetch), its q | k | v from
// q + b * q_stride, its (cos, sin) pairs from rope_tab + b * 256, its output goes to out + b * heads * 256; no quantised image.
// P.skip_store (the draft step: the rows of ONE slot are in the cache already, k_draft_kv_store): nobody writes, a Q8 cache still
// round-trips the row's own k and v in LDS, rows pos0 .. pos - 1 are history like any other.  Every cache request is clamped to the
// row's own last cached row (pos - 1): a workgroup never touches row pos of the cache -- the writer head of its group may be storing it
// -- nor a row past its context, which in a batched step may belong to nobody.
// The table entry is the one thing k_dec_attn256 does not wait for: the first pass's rows cannot be requested before it is known
// (another row's cache, another clamp).  The leading scalar arguments -- q | k | v, the table (P.batch_rows), the head counts, the row
// stride (P.q_stride) -- are preloaded into SGPRs, so the entry is a 20-byte scalar fetch issued with the kernel's first instructions,
// next to the requests for the row's q | k | v values, which hang on those arguments alone: one scalar round trip in front of the
// first cache request, not two (docs/decode_batch_heads256.md).
template <bool Q8>
__global__ void __launch_bounds__(256) k_dec_attn256_batch(const half_t *pq, const DecAttnBatchRow *prows, int pheads, int pkvh, int pq_stride,
                                                           const DecAttnParams P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HD = D256, DG = HD / 8, NSPLIT = 256 / DG;       // 32 threads per V row, 8 key residues
    half_t *qs = reinterpret_cast<half_t *>(smem);
    half_t *kn = qs + HD;
    half_t *vn = kn + HD;
    float *red = reinterpret_cast<float *>(vn + HD);               // [16]
    float *opart = red + 16;                                       // [NSPLIT][HD]
    half_t *S = reinterpret_cast<half_t *>(opart + NSPLIT * HD);   // [n_ctx]
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ql = tid & 3, qk = tid >> 2;                         // quad lane, key of the pass
    const int group = pheads / pkvh, kvh = h / group;
    const size_t row_bytes = Q8 ? (size_t)pkvh * (HD / 32) * 34 : (size_t)pkvh * HD * 2;
    const size_t head_off = Q8 ? (size_t)kvh * (HD / 32) * 34 : (size_t)kvh * HD * 2;

    // ---- the table entry (uniform: one scalar fetch, as in dec_attn_body), behind it -- in program order, not in time -- the row's values
    const DecAttnBatchRow br = prows[b];
    const half_t *qrow = pq + (size_t)b * pq_stride;
    const half_t q_in = qrow[(size_t)h * HD + tid], k_in = qrow[(size_t)(pheads + kvh) * HD + tid], v_in = qrow[(size_t)(pheads + pkvh + kvh) * HD + tid];
    float rope_c = 1.0f, rope_s = 0.0f;
    {
        const int c = tid < HD / 2 ? tid : tid - HD / 2;
        const float *rt = P.rope_tab ? P.rope_tab + (size_t)b * HD : reinterpret_cast<const float *>(qrow);      // (a valid dummy address without RoPE)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 cs = *IFA_GP(f32x2, rt + 2 * c);
        if (P.rope_order != 0) { rope_c = cs[0]; rope_s = cs[1]; }
    }
    const uint8_t *const pkc = br.kc, *const pvc = br.vc;
    const int n_ctx = br.n_ctx, pos = n_ctx - 1;
    const int jlast = max(pos - 1, 0);                             // the row's last cached row: the clamp of every request
    const bool writer = (h % group) == 0 && !P.skip_store;
    Dec256Key<Q8> kcur, knxt;
    dec256_load_key<Q8>(kcur, pkc + (size_t)min(qk, jlast) * row_bytes + head_off, ql);
    // (skip_store: store = true still runs a Q8 cache's round trip in LDS; `writer` false keeps the cache as k_draft_kv_store left it)
    dec256_stage_new<Q8>(qs, kn, vn, q_in, k_in, v_in, rope_c, rope_s, P, const_cast<uint8_t *>(pkc), const_cast<uint8_t *>(pvc),
                         (size_t)pos * row_bytes + head_off, true, writer);

    // ---- scores: a quad per key, 64 keys per pass
    half8_t qreg[8];
    dec256_lds_share<Q8>(qreg, qs, ql);
    const float alpha = 1.0f / sqrtf((float)HD) / P.kq_scale;
    const float mk = P.alibi ? alibi_slope(h + P.alibi_base, P.alibi_total) : 0.0f;
    float lmax = -INFINITY;
    for (int jb = 0; jb < n_ctx; jb += D256_PASS) {
        const int j = jb + qk;
        dec256_load_key<Q8>(knxt, pkc + (size_t)min(j + D256_PASS, jlast) * row_bytes + head_off, ql);
        half8_t kh[8];
        if (j == pos) dec256_lds_share<Q8>(kh, kn, ql);       // the row's own (round-tripped) key never leaves the LDS
        else dec256_key_halves<Q8>(kh, kcur);
        const float c = dec256_quad_dot(qreg, kh);
        if (ql == 0 && j < n_ctx) {
            half_t s = f2h(alpha * c);
            if (P.alibi) { float a = (float)j * mk; s = f2h(a + h2f(s)); }
            S[j] = s;
            lmax = fmaxf(lmax, P.kq_scale * h2f(s));
        }
        kcur = knxt;
    }
    const float acc = dec256_softmax_pv<Q8>(S, red, opart, vn, pvc, row_bytes, head_off, n_ctx, lmax, P.kq_scale);
    P.out[((size_t)b * pheads + h) * HD + tid] = f2h(acc);
}

// Keys split over workgroups, grid (heads, nsplits): k_dec_attn_scores' contract (DecAttnSplitWs: S [heads][max_ctx], lmax
// [heads][nsplits]; RoPE, the store of row p and its Q8 round trip by the split that owns it) with the quad mapping.  The rows go
// straight into the quad's registers -- the requests are whole 64-byte pieces already, so nothing is staged through LDS and the
// launch needs 16 bytes of dynamic LDS (dec_attn_scores_smem) instead of the 132 KiB a 256-row stage of 256-wide F16 rows would take.
template <bool Q8>
__global__ void __launch_bounds__(256) k_dec_attn256_scores(const DecAttnParams P, const DecAttnSplitWs ws)
{
    constexpr int HD = D256;
    __shared__ __attribute__((aligned(16))) half_t qs[HD];
    __shared__ __attribute__((aligned(16))) half_t kn[HD];
    __shared__ __attribute__((aligned(16))) half_t vn[HD];
    __shared__ float red[4];
    const int h = blockIdx.x, sidx = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = tid & 3, qk = tid >> 2;
    const int pos = *(const __attribute__((address_space(4))) int *)(P.state + 1), n_ctx = pos + 1;
    int j0, j1; dec_split_range(n_ctx, ws.nsplits, sidx, j0, j1);
    const int group = P.heads / P.kv_heads, kvh = h / group;
    const bool has_new = pos >= j0 && pos < j1;             // this split owns the new token's row
    const bool writer = has_new && (h % group) == 0;
    const size_t row_bytes = Q8 ? (size_t)P.kv_heads * (HD / 32) * 34 : (size_t)P.kv_heads * HD * 2;
    const size_t head_off = Q8 ? (size_t)kvh * (HD / 32) * 34 : (size_t)kvh * HD * 2;
    const int jlast = max(min(j1, pos) - 1, 0);             // the last cached row of this split (clamp of every request)

    const half_t q_in = P.q[(size_t)h * HD + tid], k_in = P.k_new[(size_t)kvh * HD + tid], v_in = P.v_new[(size_t)kvh * HD + tid];
    float rope_c = 1.0f, rope_s = 0.0f;
    {
        const int c = tid < HD / 2 ? tid : tid - HD / 2;
        const float *rt = P.rope_tab ? P.rope_tab : reinterpret_cast<const float *>(P.q);      // (a valid dummy address without RoPE)
        const float c0v = rt[2 * c], s0v = rt[2 * c + 1];
        if (P.rope_order != 0) { rope_c = c0v; rope_s = s0v; }
    }
    Dec256Key<Q8> kcur, knxt;
    dec256_load_key<Q8>(kcur, P.kcache + (size_t)min(j0 + qk, jlast) * row_bytes + head_off, ql);
    dec256_stage_new<Q8>(qs, kn, vn, q_in, k_in, v_in, rope_c, rope_s, P, P.kcache, P.vcache, (size_t)pos * row_bytes + head_off, has_new, writer);

    half8_t qreg[8];
    dec256_lds_share<Q8>(qreg, qs, ql);
    const float alpha = 1.0f / sqrtf((float)HD) / P.kq_scale;
    const float mk = P.alibi ? alibi_slope(h + P.alibi_base, P.alibi_total) : 0.0f;
    float lmax = -INFINITY;
    for (int jb = j0; jb < j1; jb += D256_PASS) {
        const int j = jb + qk;
        dec256_load_key<Q8>(knxt, P.kcache + (size_t)min(j + D256_PASS, jlast) * row_bytes + head_off, ql);
        half8_t kh[8];
        if (j == pos) dec256_lds_share<Q8>(kh, kn, ql);
        else dec256_key_halves<Q8>(kh, kcur);
        const float c = dec256_quad_dot(qreg, kh);
        if (ql == 0 && j < j1) {
            half_t sv = f2h(alpha * c);
            if (P.alibi) { float a = (float)j * mk; sv = f2h(a + h2f(sv)); }
            ws.S[(size_t)h * P.max_ctx + j] = sv;
            lmax = fmaxf(lmax, P.kq_scale * h2f(sv));
        }
        kcur = knxt;
    }
    lmax = wave_max(lmax);
    if (lane == 0) red[wave] = lmax;
    __syncthreads();
    if (tid == 0) ws.lmax[h * ws.nsplits + sidx] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

} // namespace ifa
