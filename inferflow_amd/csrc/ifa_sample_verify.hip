// ifa_sample_verify.hip -- the verify step of lookup decoding for seeded, sampled queries: the rows of a draft step drawn as a
// chain.  Row 0 is drawn with the query's generator; row i + 1 was computed behind the guess draft[i], so it counts only if row
// i's draw IS that guess; the chain ends at the first draw that differs (that draw is still a valid token).  The draw of the
// sampled strategies always advances the 48-bit generator by exactly two steps (sr_draw: one sr_next_double, whatever the cut
// length), so row i's state is known up front: the query's state 2 i steps on.  The result is therefore exactly what a row-by-row
// loop of ifa_sample_pool_host over the same pools emits -- no rejection sampling, no approximation:
//
//   st = *rng; e = 0
//   for i in 0 .. rows-1:
//       draw row i by the rule of ifa_sample_pool_host with state st -> (tok, st')            (greedy: ids[i][0], st' = st)
//       if the row cannot be drawn (empty pool, NaN, unknown strategy): if *err == 0: *err = i + 1; break
//       tokens[e++] = tok; st = st'
//       if i == rows-1 or tok != draft[i]: break
//   *rng = st; *n_out = e; tokens[e..rows) = -1
//
// A row behind the first mismatch is never looked at: it can neither raise an error nor move the generator.
//
// k_sample_verify: ONE workgroup of `rows` waves (rows <= 8).  Wave i jumps the state 2 i steps (at most 14 multiply-adds of
// sr_next's recurrence) and draws row i with sample_row (csrc/ifa_sample_wave.h: the pool in the wave's registers, as in
// k_sample_pool) -- all rows in parallel, every draw speculative.  Token, index, ok flag and the row's draft token go to LDS;
// behind one workgroup barrier lane 0 of wave 0 walks the at most 8 entries by the rule above -- LDS reads only: a draft token
// loaded inside the walk would put one memory round trip per accepted row on the critical path -- and writes the outputs and the
// state 2 e steps on.  ifa_sample_verify_host is the same chain on the CPU, built on ifa_sample_pool_host: the reference, bit for bit.
#include <algorithm>
#include "ifa_host.h"
#include "ifa_sample_wave.h"

namespace ifa {

constexpr int SV_ROWS = 8;

// the LCG of sr_next, `steps` times (the draw's own steps, restated without the output bits)
IFA_SR_HD uint64_t sv_advance(uint64_t st, int steps)
{
    for (int j = 0; j < steps; j++) st = (st * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1ULL);
    return st;
}

__global__ void __launch_bounds__(512) k_sample_verify(const int *__restrict__ counts, const int *__restrict__ ids, const uint16_t *__restrict__ vals,
                                                       int rows, int k_stride, const ifa_sample_params *__restrict__ params,
                                                       const int *__restrict__ draft, unsigned long long *__restrict__ rng,
                                                       int *__restrict__ tokens_out, int *__restrict__ index_out, int *__restrict__ n_out,
                                                       int *__restrict__ err)
{
    __shared__ int s_tok[SV_ROWS], s_idx[SV_ROWS], s_ok[SV_ROWS], s_draft[SV_ROWS];
    const int row = sr_uni((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int strategy = sr_uni(params->strategy_id), max_k = sr_uni(params->max_k);
    // (everything the scan behind the barrier needs is loaded here, under the draw: the scan itself makes no memory round trip)
    const uint64_t st0 = sr_uni64(*rng);
    if (row < rows) {
        const int guess = row < rows - 1 ? sr_uni(draft[row]) : -1;
        const size_t base = (size_t)row * (size_t)k_stride;
        const int n = min(max(sr_uni(counts[row]), 0), min(k_stride, SR_MAX));
        const float temperature = sr_unif(params->temperature), top_p = sr_unif(params->top_p), min_p = sr_unif(params->min_p);
        int token = -1, index = -1;
        bool ok = n > 0 && sr_strategy_ok(strategy);
        if (ok && strategy == SR_GREEDY) { token = sr_uni(ids[base]); index = 0; }
        else if (ok) {
            const uint64_t st = sv_advance(st0, 2 * row);
            if (n <= 64) (void)sample_row<1>(n, lane, base, ids, vals, strategy, temperature, top_p, max_k, min_p, st, nullptr, token, index, ok);
            else (void)sample_row<4>(n, lane, base, ids, vals, strategy, temperature, top_p, max_k, min_p, st, nullptr, token, index, ok);
        }
        if (lane == 0) { s_tok[row] = ok ? token : -1; s_idx[row] = ok ? index : -1; s_ok[row] = ok ? 1 : 0; s_draft[row] = guess; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int e = 0;
    for (int i = 0; i < rows; i++) {
        if (!s_ok[i]) { if (*err == 0) *err = i + 1; break; }
        const int tok = s_tok[i];
        tokens_out[e] = tok;
        if (index_out) index_out[e] = s_idx[i];
        e++;
        if (i == rows - 1 || tok != s_draft[i]) break;
    }
    for (int i = e; i < rows; i++) {
        tokens_out[i] = -1;
        if (index_out) index_out[i] = -1;
    }
    *n_out = e;
    if (strategy != SR_GREEDY && e > 0) *rng = (unsigned long long)sv_advance(st0, 2 * e);
}

// engine-internal: the launch
int sample_verify_launch(const int *counts, const int *ids, const void *vals, int rows, int k_stride, const ifa_sample_params *params, const int *draft,
                         unsigned long long *rng, int *tokens_out, int *index_out, int *n_out, int *err, hipStream_t s)
{
    k_sample_verify<<<dim3(1), dim3(64u * (unsigned)rows), 0, s>>>(counts, ids, (const uint16_t *)vals, rows, k_stride, params, draft, rng, tokens_out,
                                                                   index_out, n_out, err);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifa

extern "C" {

int ifa_sample_verify_rows(const int *counts_dev, const int *ids_dev, const void *vals_f16_dev, size_t rows, int k_stride,
                           const ifa_sample_params *params_dev, const int *draft_dev, unsigned long long *rng_state_dev, int *tokens_out_dev,
                           int *index_out_dev, int *n_out_dev, int *err_dev, ifa_stream stream)
{
    IFA_REQUIRE(counts_dev && ids_dev && vals_f16_dev && params_dev && rng_state_dev && tokens_out_dev && n_out_dev && err_dev, "ifa_sample_verify_rows: null pointer");
    IFA_REQUIRE(rows >= 1 && rows <= (size_t)ifa::SV_ROWS, "ifa_sample_verify_rows: rows %zu outside 1..%d", rows, ifa::SV_ROWS);
    IFA_REQUIRE(rows == 1 || draft_dev, "ifa_sample_verify_rows: %zu rows without draft tokens", rows);
    IFA_REQUIRE(k_stride >= 1 && k_stride <= IFA_POOL_MAX, "ifa_sample_verify_rows: k_stride %d outside 1..%d", k_stride, IFA_POOL_MAX);
    return ifa::sample_verify_launch(counts_dev, ids_dev, vals_f16_dev, (int)rows, k_stride, params_dev, draft_dev, rng_state_dev, tokens_out_dev,
                                     index_out_dev, n_out_dev, err_dev, ifa_s(stream));
}

// host-only: the same chain on the CPU, one ifa_sample_pool_host per reached row
int ifa_sample_verify_host(const int *counts, const int *ids, const unsigned short *vals_f16, int rows, int k_stride, const ifa_sample_params *p,
                           const int *draft, unsigned long long *rng_state_inout, int *tokens_out, int *index_out, int *n_out, int *err_inout)
{
    IFA_REQUIRE(counts && ids && vals_f16 && p && rng_state_inout && tokens_out && n_out && err_inout, "ifa_sample_verify_host: null pointer");
    IFA_REQUIRE(rows >= 1 && rows <= ifa::SV_ROWS, "ifa_sample_verify_host: rows %d outside 1..%d", rows, ifa::SV_ROWS);
    IFA_REQUIRE(rows == 1 || draft, "ifa_sample_verify_host: %d rows without draft tokens", rows);
    IFA_REQUIRE(k_stride >= 1 && k_stride <= IFA_POOL_MAX, "ifa_sample_verify_host: k_stride %d outside 1..%d", k_stride, IFA_POOL_MAX);
    unsigned long long st = *rng_state_inout;
    int e = 0;
    for (int i = 0; i < rows; i++) {
        const size_t base = (size_t)i * (size_t)k_stride;
        const int n = std::min(std::max(counts[i], 0), std::min(k_stride, (int)IFA_POOL_MAX));
        int tok = -1, idx = -1;
        unsigned long long next = st;
        // (every refusal of the one-row rule -- empty pool, NaN, unknown strategy -- is a row that cannot be drawn)
        if (ifa_sample_pool_host(ids + base, vals_f16 + base, n, p, &next, &tok, &idx, nullptr, nullptr, nullptr) != IFA_OK) {
            if (*err_inout == 0) *err_inout = i + 1;
            break;
        }
        tokens_out[e] = tok;
        if (index_out) index_out[e] = idx;
        e++; st = next;
        if (i == rows - 1 || tok != draft[i]) break;
    }
    for (int i = e; i < rows; i++) {
        tokens_out[i] = -1;
        if (index_out) index_out[i] = -1;
    }
    *rng_state_inout = st;
    *n_out = e;
    return IFA_OK;
}

} // extern "C"
