// ifa_logit_adjust.hip -- logit processors on the device: repetition / frequency / presence penalties and logit_bias, applied to
// the F16 logits rows of a step before the candidate pool (ifa_topk_pool.hip) and the log-sum-exp (ifa_logprob.hip) read them.
//
// State per slot (a slot = one query), dense over the vocabulary of n ids:
//   state[slot][n]  u32   bit 31: the id occurs in the prompt; bits 0..30: how many times the id has been generated
//   bias[slot][n]   f32   logit_bias, 0 where none is set, -inf bans the id
//   params[slot]    3 f32 {rep, freq, pres}
//
// Arithmetic per id, fp32, every operation rounded on its own (no contraction), in this order:
//   1. x = float(in[id]); w = state[q][id]; c = w & 0x7fffffff
//   2. w != 0 && rep != 1:  x = x > 0 ? x / rep : x * rep            (the HF rule, over prompt + generated ids)
//   3. x = x - (freq * float(c) + (c > 0 ? pres : 0))                 (the OpenAI rule, over generated ids only)
//   4. x = x + bias[q][id]
//   5. bias[q][id] == -inf: -inf.  Else clamp to +-65504 and round to F16 (RNE); a NaN is written as 0x7E00.
// Consequences of taking the steps literally: an infinite input comes out as +-65504, and a -0.0 input under neutral parameters
// comes out as +0.0 (-0 + +0 under RNE) -- the pool and the log-sum-exp treat the two zeros alike.
//
// The work is element-wise: a row is split over workgroups, grid (ceil(n / 2048), rows), 256 threads (4 waves), 8 ids per thread
// as ONE 16-byte load of halfs + 2 x 4 state words + 2 x 4 bias words and one 16-byte store.  That takes the four row bases
// (input, output, state, bias) 16-byte aligned -- so whenever n and the row stride are multiples of 8 (every real vocabulary; the
// worker's buffers always) -- with the n % 8 ids behind the last vector going one by one; a row with any base off a boundary (odd
// n or stride) goes one id per thread and step.  No LDS, no atomics, no reduction: run-to-run identical.
//
// ifa_logit_adjust_draft_rows is the same arithmetic (one inline function, la_one) for the rows of ONE slot's draft step: row r sees
// the state words as they would be after ifa_logit_state_add of draft[0..r) -- w' = w + #{j < r : draft[j] == id} -- and writes no
// state.  Same grid, same 16-byte / id-by-id paths.
//
// The two state kernels use integer vector atomics (atomicOr for the prompt bit -- duplicates are the normal case -- and atomicAdd
// for the counts): integer addition commutes, the result is deterministic.
#include <algorithm>
#include <cmath>
#include "ifa_host.h"
#include "ifa_device.h"

namespace ifa {

constexpr int LA_THREADS = 256, LA_PER_WG = LA_THREADS * 8;
constexpr unsigned LA_PROMPT_BIT = 0x80000000u, LA_COUNT_MASK = 0x7fffffffu;

__device__ __forceinline__ uint16_t la_one(uint16_t in, unsigned w, float b, float rep, float freq, float pres)
{
    float x = hbits2f(in);
    const unsigned c = w & LA_COUNT_MASK;
    if (w != 0u && rep != 1.0f) x = x > 0.0f ? __fdiv_rn(x, rep) : __fmul_rn(x, rep);
    x = __fsub_rn(x, __fadd_rn(__fmul_rn(freq, (float)c), c > 0u ? pres : 0.0f));
    x = __fadd_rn(x, b);
    if (b == -INFINITY) return (uint16_t)0xFC00u;
    if (x != x) return (uint16_t)0x7E00u;
    return f2hbits(fminf(fmaxf(x, -65504.0f), 65504.0f));
}

// The draft step (ifa_logit_adjust_draft_rows): row r of a slot is adjusted as if draft[0..r) had been counted already,
//   w' = w + #{j < r : draft[j] == id}
// (bit 31 is kept, the count is w' & 0x7fffffff, the repetition rule fires on w' != 0), then la_one as ever.  dn = 0: w' = w.
constexpr int LA_DRAFT_MAX = 7;
struct LaDraft { int dn; int d[LA_DRAFT_MAX]; };

template <bool DRAFT> __device__ __forceinline__ unsigned la_word(unsigned w, int id, const LaDraft &D)
{
    if constexpr (DRAFT) {
#pragma unroll
        for (int j = 0; j < LA_DRAFT_MAX; j++) w += (j < D.dn && D.d[j] == id) ? 1u : 0u;
    }
    return w;
}

// one row of the grid (ceil(n / 2048), rows): chunk blockIdx.x of the row at in_row / out_row with the slot's st / bs rows
template <bool DRAFT>
__device__ __forceinline__ void la_row_chunk(const uint16_t *__restrict__ in_row, uint16_t *__restrict__ out_row, const unsigned *__restrict__ st,
                                             const float *__restrict__ bs, int n, float rep, float freq, float pres, const LaDraft &D)
{
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const bool aligned = (((uintptr_t)in_row | (uintptr_t)out_row | (uintptr_t)st | (uintptr_t)bs) & 15u) == 0;
    if (!aligned) {                     // (uniform per row) one id per thread and step, coalesced
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int id = chunk * LA_PER_WG + e * LA_THREADS + tid;
            if (id < n) out_row[id] = la_one(in_row[id], la_word<DRAFT>(st[id], id, D), bs[id], rep, freq, pres);
        }
        return;
    }
    const int nvec = n >> 3, tail0 = nvec << 3;
    if (chunk == (int)gridDim.x - 1 && tail0 + tid < n) {
        const int id = tail0 + tid;
        out_row[id] = la_one(in_row[id], la_word<DRAFT>(st[id], id, D), bs[id], rep, freq, pres);
    }
    const int v = chunk * LA_THREADS + tid;
    if (v >= nvec) return;
    const int id0 = v << 3;
    const uint4 xi = *reinterpret_cast<const uint4 *>(in_row + id0);
    const uint4 w0 = *reinterpret_cast<const uint4 *>(st + id0), w1 = *reinterpret_cast<const uint4 *>(st + id0 + 4);
    const float4 b0 = *reinterpret_cast<const float4 *>(bs + id0), b1 = *reinterpret_cast<const float4 *>(bs + id0 + 4);
    const unsigned xw[4] = {xi.x, xi.y, xi.z, xi.w};
    const unsigned w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    unsigned o[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const unsigned lo = la_one((uint16_t)(xw[p] & 0xFFFFu), la_word<DRAFT>(w[2 * p], id0 + 2 * p, D), b[2 * p], rep, freq, pres);
        const unsigned hi = la_one((uint16_t)(xw[p] >> 16), la_word<DRAFT>(w[2 * p + 1], id0 + 2 * p + 1, D), b[2 * p + 1], rep, freq, pres);
        o[p] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4 *>(out_row + id0) = make_uint4(o[0], o[1], o[2], o[3]);
}

// grid (ceil(n / 2048), rows)
__global__ void __launch_bounds__(LA_THREADS) k_logit_adjust(const uint16_t *__restrict__ logits, size_t row_stride, const int *__restrict__ row_idx,
                                                             const int *__restrict__ state_slot, int n, const unsigned *__restrict__ state,
                                                             const float *__restrict__ bias, const float *__restrict__ params,
                                                             uint16_t *__restrict__ out)
{
    const int r = blockIdx.y;
    const size_t src_row = row_idx ? (size_t)row_idx[r] : (size_t)r;
    const size_t q = (size_t)state_slot[r];
    LaDraft D;
    D.dn = 0;
    la_row_chunk<false>(logits + src_row * row_stride, out + (size_t)r * (size_t)n, state + q * (size_t)n, bias + q * (size_t)n, n, params[q * 3],
                        params[q * 3 + 1], params[q * 3 + 2], D);
}

// grid (ceil(n / 2048), rows): the rows of ONE slot's draft step, row r behind draft[0..r)
__global__ void __launch_bounds__(LA_THREADS) k_logit_adjust_draft(const uint16_t *__restrict__ logits, size_t row_stride, const int *__restrict__ state_slot,
                                                                   int n, const int *__restrict__ draft, const unsigned *__restrict__ state,
                                                                   const float *__restrict__ bias, const float *__restrict__ params,
                                                                   uint16_t *__restrict__ out)
{
    const int r = blockIdx.y;
    const size_t q = (size_t)state_slot[0];
    LaDraft D;
    D.dn = min(r, LA_DRAFT_MAX);
#pragma unroll
    for (int j = 0; j < LA_DRAFT_MAX; j++) D.d[j] = j < D.dn ? draft[j] : -1;
    la_row_chunk<true>(logits + (size_t)r * row_stride, out + (size_t)r * (size_t)n, state + q * (size_t)n, bias + q * (size_t)n, n, params[q * 3],
                       params[q * 3 + 1], params[q * 3 + 2], D);
}

// after the slot's two rows have been cleared: the prompt bit of every prompt id, the bias entries, the parameters
__global__ void __launch_bounds__(LA_THREADS) k_logit_state_fill(int slot, const int *__restrict__ prompt, int n_prompt, float rep, float freq, float pres,
                                                                 const int *__restrict__ bias_ids, const float *__restrict__ bias_vals, int n_bias,
                                                                 int n, unsigned *__restrict__ state, float *__restrict__ bias, float *__restrict__ params)
{
    const int i = blockIdx.x * LA_THREADS + threadIdx.x;
    const size_t base = (size_t)slot * (size_t)n;
    if (i < n_prompt) {
        const int t = prompt[i];
        if (t >= 0 && t < n) atomicOr(&state[base + (size_t)t], LA_PROMPT_BIT);
    }
    if (i < n_bias) {
        const int t = bias_ids[i];
        if (t >= 0 && t < n) bias[base + (size_t)t] = bias_vals[i];
    }
    if (i == 0) { params[(size_t)slot * 3] = rep; params[(size_t)slot * 3 + 1] = freq; params[(size_t)slot * 3 + 2] = pres; }
}

__global__ void __launch_bounds__(LA_THREADS) k_logit_state_add(const int *__restrict__ slots, const int *__restrict__ tokens, int n_pairs, int n,
                                                                int n_slots, unsigned *__restrict__ state)
{
    const int i = blockIdx.x * LA_THREADS + threadIdx.x;
    if (i >= n_pairs) return;
    const int s = slots[i], t = tokens[i];
    if (s >= 0 && s < n_slots && t >= 0 && t < n) atomicAdd(&state[(size_t)s * (size_t)n + (size_t)t], 1u);
}

int logit_adjust_rows(const void *logits, size_t row_stride, const int *row_idx_dev, const int *state_slot_dev, size_t rows, size_t n,
                      const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s)
{
    k_logit_adjust<<<dim3(ifa_cdiv(n, LA_PER_WG), (unsigned)rows), dim3(LA_THREADS), 0, s>>>((const uint16_t *)logits, row_stride, row_idx_dev, state_slot_dev,
                                                                                             (int)n, state_dev, bias_dev, params_dev, (uint16_t *)out);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

int logit_adjust_draft_rows(const void *logits, size_t row_stride, const int *state_slot_dev, size_t rows, size_t n, const int *draft_dev,
                            const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s)
{
    k_logit_adjust_draft<<<dim3(ifa_cdiv(n, LA_PER_WG), (unsigned)rows), dim3(LA_THREADS), 0, s>>>((const uint16_t *)logits, row_stride, state_slot_dev, (int)n,
                                                                                                   draft_dev, state_dev, bias_dev, params_dev, (uint16_t *)out);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifa

extern "C" {

int ifa_logit_adjust_rows(const void *logits_f16, size_t row_stride, const int *row_idx_dev, const int *state_slot_dev, size_t rows, size_t n,
                          const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out_f16_dev, ifa_stream stream)
{
    IFA_REQUIRE(logits_f16 && state_slot_dev && state_dev && bias_dev && params_dev && out_f16_dev, "ifa_logit_adjust_rows: null pointer");
    IFA_REQUIRE(n > 0 && n < 0x7FFFFFFFu && row_stride >= n, "ifa_logit_adjust_rows: n %zu, row stride %zu", n, row_stride);
    IFA_REQUIRE(rows > 0 && rows <= 65535, "ifa_logit_adjust_rows: rows %zu", rows);
    IFA_REQUIRE(logits_f16 != out_f16_dev, "ifa_logit_adjust_rows: the op is out of place");
    return ifa::logit_adjust_rows(logits_f16, row_stride, row_idx_dev, state_slot_dev, rows, n, state_dev, bias_dev, params_dev, out_f16_dev, ifa_s(stream));
}

int ifa_logit_adjust_draft_rows(const void *logits_f16, size_t row_stride, const int *state_slot_dev, size_t rows, size_t n, const int *draft_dev,
                                const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out_f16_dev, ifa_stream stream)
{
    IFA_REQUIRE(logits_f16 && state_slot_dev && state_dev && bias_dev && params_dev && out_f16_dev, "ifa_logit_adjust_draft_rows: null pointer");
    IFA_REQUIRE(n > 0 && n < 0x7FFFFFFFu && row_stride >= n, "ifa_logit_adjust_draft_rows: n %zu, row stride %zu", n, row_stride);
    IFA_REQUIRE(rows >= 1 && rows <= (size_t)ifa::LA_DRAFT_MAX + 1, "ifa_logit_adjust_draft_rows: rows %zu outside 1..%d", rows, ifa::LA_DRAFT_MAX + 1);
    IFA_REQUIRE(rows == 1 || draft_dev, "ifa_logit_adjust_draft_rows: %zu rows without draft tokens", rows);
    IFA_REQUIRE(logits_f16 != out_f16_dev, "ifa_logit_adjust_draft_rows: the op is out of place");
    return ifa::logit_adjust_draft_rows(logits_f16, row_stride, state_slot_dev, rows, n, draft_dev, state_dev, bias_dev, params_dev, out_f16_dev, ifa_s(stream));
}

int ifa_logit_state_reset(int slot, const int *prompt_tokens_dev, size_t n_prompt, float rep, float freq, float pres, const int *bias_ids_dev,
                          const float *bias_vals_dev, size_t n_bias, size_t n, unsigned *state_dev, float *bias_dev, float *params_dev, ifa_stream stream)
{
    IFA_REQUIRE(state_dev && bias_dev && params_dev, "ifa_logit_state_reset: null pointer");
    IFA_REQUIRE(slot >= 0 && n > 0 && n < 0x7FFFFFFFu, "ifa_logit_state_reset: slot %d, n %zu", slot, n);
    IFA_REQUIRE(n_prompt < 0x7FFFFFFFu && (n_prompt == 0 || prompt_tokens_dev), "ifa_logit_state_reset: %zu prompt tokens without a pointer", n_prompt);
    IFA_REQUIRE(n_bias < 0x7FFFFFFFu && (n_bias == 0 || (bias_ids_dev && bias_vals_dev)), "ifa_logit_state_reset: %zu bias entries without pointers", n_bias);
    hipStream_t s = ifa_s(stream);
    IFA_HIP_CHECK(hipMemsetAsync(state_dev + (size_t)slot * n, 0, n * sizeof(unsigned), s));
    IFA_HIP_CHECK(hipMemsetAsync(bias_dev + (size_t)slot * n, 0, n * sizeof(float), s));
    const size_t work = std::max<size_t>(std::max(n_prompt, n_bias), 1);
    ifa::k_logit_state_fill<<<dim3(ifa_cdiv(work, ifa::LA_THREADS)), dim3(ifa::LA_THREADS), 0, s>>>(slot, prompt_tokens_dev, (int)n_prompt, rep, freq, pres, bias_ids_dev,
                                                                                                   bias_vals_dev, (int)n_bias, (int)n, state_dev, bias_dev, params_dev);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

int ifa_logit_state_add(const int *slots_dev, const int *tokens_dev, size_t n_pairs, size_t n, size_t n_slots, unsigned *state_dev, ifa_stream stream)
{
    IFA_REQUIRE(n_pairs == 0 || (slots_dev && tokens_dev && state_dev), "ifa_logit_state_add: null pointer");
    IFA_REQUIRE(n > 0 && n < 0x7FFFFFFFu && n_slots > 0 && n_slots < 0x7FFFFFFFu && n_pairs < 0x7FFFFFFFu, "ifa_logit_state_add: n %zu, slots %zu, pairs %zu", n, n_slots, n_pairs);
    if (n_pairs == 0) return IFA_OK;
    ifa::k_logit_state_add<<<dim3(ifa_cdiv(n_pairs, ifa::LA_THREADS)), dim3(ifa::LA_THREADS), 0, ifa_s(stream)>>>(slots_dev, tokens_dev, (int)n_pairs, (int)n, (int)n_slots, state_dev);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // extern "C"
