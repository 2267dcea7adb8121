// ifa_sample_pool.hip -- the draw of the sampled strategies on the device: one wave per row reads the candidate pool that
// k_topk_pool wrote (count, ids, F16 values; csrc/ifa_topk_pool.hip) and runs the rule of csrc/ifa_sample_rule.h -- std::sort's
// tie order, SoftMaxPool, the top_p / top_k / min_p cut, DrawOne with the query's 48-bit generator -- so a sampled step needs no
// copy of the pool to the host.  The same header compiled for the host is ifa_sample_pool_host, the reference the tests compare
// this kernel with bit for bit.
//
// The pool in the registers of the wave and the draw of one row on it are csrc/ifa_sample_wave.h, shared with k_sample_verify
// (ifa_sample_verify.hip): no LDS, no dependent memory round trips, every loop bounded by the pool length.
#include "ifa_host.h"
#include "ifa_sample_wave.h"

namespace ifa {

using namespace ifa_sr;

// ---- the pool in host arrays
struct SrHostPool {
    sr_item it[SR_MAX];
    int stk[SR_STACK];
    double base[SR_MAX];
    sr_item get(int i) const { return it[i]; }
    void set(int i, sr_item v) { it[i] = v; }
    int stk_get(int j) const { return stk[j]; }
    void stk_set(int j, int v) { stk[j] = v; }
    double base_get(int i) const { return base[i]; }
    void base_set(int i, double v) { base[i] = v; }
};

// One wave per row.  state == nullptr: the op (row = blockIdx.x, error code row + 1).  state != nullptr: the tail of a decode
// step on its one row -- the draw, then exactly what k_dec_argmax_advance does to the device state (token ring, token, position,
// step count; error code step + 1).  A row that cannot be drawn (empty pool, unknown strategy, a NaN weight -- k_topk_pool never
// offers one) stores its code into *err if no earlier code is there, token / index -1, and leaves its generator alone.
__global__ void __launch_bounds__(64) k_sample_pool(const int *__restrict__ counts, const int *__restrict__ ids, const uint16_t *__restrict__ vals,
                                                    int k_stride, const ifa_sample_params *__restrict__ params, unsigned long long *__restrict__ rng,
                                                    int *__restrict__ tokens_out, int *__restrict__ index_out, float *__restrict__ weights_out,
                                                    int *__restrict__ err, int *__restrict__ state, int ring)
{
    const int row = (int)blockIdx.x, lane = (int)threadIdx.x;
    const size_t base = (size_t)row * (size_t)k_stride;
    const int n = min(max(sr_uni(counts[row]), 0), min(k_stride, SR_MAX));
    const int strategy = sr_uni(params[row].strategy_id), max_k = sr_uni(params[row].max_k);
    const float temperature = sr_unif(params[row].temperature), top_p = sr_unif(params[row].top_p), min_p = sr_unif(params[row].min_p);
    int token = -1, index = -1;
    bool ok = n > 0 && sr_strategy_ok(strategy);
    if (ok && strategy == SR_GREEDY) { token = sr_uni(ids[base]); index = 0; }
    else if (ok) {
        uint64_t st = sr_uni64(rng[row]);
        st = n <= 64 ? sample_row<1>(n, lane, base, ids, vals, strategy, temperature, top_p, max_k, min_p, st, weights_out, token, index, ok)
                     : sample_row<4>(n, lane, base, ids, vals, strategy, temperature, top_p, max_k, min_p, st, weights_out, token, index, ok);
        if (ok && lane == 0) rng[row] = (unsigned long long)st;
    }
    if (!ok) { token = -1; index = -1; }
    if (lane == 0) {
        int step = 0;
        if (state) step = state[2];
        if (!ok) atomicCAS(err, 0, state ? step + 1 : row + 1);
        tokens_out[row] = token;
        index_out[row] = index;
        if (state) {
            const int t = ok ? token : state[0];
            state[8 + (step % ring)] = t;
            state[0] = t;
            state[1] = state[1] + 1;
            state[2] = step + 1;
        }
    }
}

// engine-internal: the launch (state == nullptr: rows of the op; else the one row of a decode step's tail)
int sample_pool_launch(const int *counts, const int *ids, const void *vals, size_t rows, int k_stride, const ifa_sample_params *params,
                       unsigned long long *rng, int *tokens_out, int *index_out, float *weights_out, int *err, int *state, int ring, hipStream_t s)
{
    k_sample_pool<<<dim3((unsigned)rows), dim3(64), 0, s>>>(counts, ids, (const uint16_t *)vals, k_stride, params, rng, tokens_out, index_out, weights_out,
                                                           err, state, ring);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifa

extern "C" {

int ifa_sample_pool_rows(const int *counts_dev, const int *ids_dev, const void *vals_f16_dev, size_t rows, int k_stride,
                         const ifa_sample_params *params_dev, unsigned long long *rng_state_dev, int *tokens_out_dev, int *index_out_dev,
                         float *weights_out_dev, int *err_dev, ifa_stream stream)
{
    IFA_REQUIRE(counts_dev && ids_dev && vals_f16_dev && params_dev && rng_state_dev && tokens_out_dev && index_out_dev && err_dev, "ifa_sample_pool_rows: null pointer");
    IFA_REQUIRE(k_stride >= 1 && k_stride <= IFA_POOL_MAX, "ifa_sample_pool_rows: k_stride %d outside 1..%d", k_stride, IFA_POOL_MAX);
    IFA_REQUIRE(rows > 0 && rows <= 65535, "ifa_sample_pool_rows: rows %zu", rows);
    return ifa::sample_pool_launch(counts_dev, ids_dev, vals_f16_dev, rows, k_stride, params_dev, rng_state_dev, tokens_out_dev, index_out_dev,
                                   weights_out_dev, err_dev, nullptr, 1, ifa_s(stream));
}

// host-only: the same rule on the CPU
int ifa_sample_pool_host(const int *ids, const unsigned short *vals_f16, int count, const ifa_sample_params *p, unsigned long long *rng_state_inout,
                         int *token_out, int *index_out, int *cut_len_out, float *weights_out, int *order_ids_out)
{
    using namespace ifa_sr;
    IFA_REQUIRE(p && rng_state_inout && token_out, "ifa_sample_pool_host: null pointer");
    IFA_REQUIRE(count >= 0 && count <= IFA_POOL_MAX && (count == 0 || (ids && vals_f16)), "ifa_sample_pool_host: count %d outside 0..%d", count, IFA_POOL_MAX);
    IFA_REQUIRE(sr_strategy_ok(p->strategy_id), "ifa_sample_pool_host: strategy %d is not one of 1 sample.std, 2 greedy, 3 top_k, 4 sample.top_p, 7 min_p", p->strategy_id);
    *token_out = -1;
    if (index_out) *index_out = -1;
    if (cut_len_out) *cut_len_out = 0;
    if (count == 0) return ifa_fail(IFA_ERR_STATE, "ifa_sample_pool_host: empty pool");
    if (p->strategy_id == SR_GREEDY) {
        *token_out = ids[0];
        if (index_out) *index_out = 0;
        if (cut_len_out) *cut_len_out = 1;
        return IFA_OK;
    }
    ifa::SrHostPool a;
    for (int i = 0; i < count; i++) {
        sr_item it;
        it.w = sr_half_bits_to_float(vals_f16[i]); it.id = ids[i];
        IFA_REQUIRE(it.w == it.w, "ifa_sample_pool_host: entry %d is NaN (the pool never offers one)", i);
        a.set(i, it);
    }
    sr_sort(a, count);
    const float m = sr_max(a, count), t = sr_temperature(p->temperature);
    for (int i = 0; i < count; i++) { sr_item it = a.get(i); it.w = sr_exp(it.w, m, t); a.set(i, it); }
    const float sum = sr_sum(a, count);
    for (int i = 0; i < count; i++) {
        sr_item it = a.get(i);
        it.w = it.w / sum;
        a.set(i, it);
        if (weights_out) weights_out[i] = it.w;
        if (order_ids_out) order_ids_out[i] = it.id;
    }
    const int len = sr_cut(a, count, p->strategy_id, p->top_p, p->max_k, p->min_p);
    uint64_t st = (uint64_t)*rng_state_inout;
    const int index = sr_draw(a, len, st);
    *rng_state_inout = (unsigned long long)st;
    *token_out = a.get(index).id;
    if (index_out) *index_out = index;
    if (cut_len_out) *cut_len_out = len;
    return IFA_OK;
}

} // extern "C"
