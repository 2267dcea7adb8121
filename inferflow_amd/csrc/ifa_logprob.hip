// ifa_logprob.hip -- the normaliser of a logits row on the device: lse = max + log(sum exp(x - max)) over the FULL row of F16
// logits (no exclusion mask: the perplexity tool's softmax, host/perplexity.cc TokenNll), fp32 arithmetic on the widened halfs,
// plus the row's value at a target id.  log p(id) = float(row[id]) - lse.
//
// A row (64 KB at 32000 ids, 300 KB at 150K) sits in L2 behind the lm_head launch.  Workgroups of 256 threads (4 waves); a
// workgroup owns a contiguous part of the row's 16-byte vectors, every lane keeps 8 sums (one per half of its vector: 2048
// independent sums per workgroup, the longest chain is ceil(vectors / 256) adds), then a fixed tree: 8 -> 1 in the lane, DPP /
// shuffles across the wave, LDS across the 4 waves.  Two passes over the part (its max, then the sum of exp(x - max)); the second
// one hits the cache.  Many rows (a prompt): one workgroup per row, finished in that launch.  Few rows (a decode step): a row is
// split over up to 64 workgroups, each leaves (max_s, sum_s), and a second launch of one wave per row combines them in a fixed
// order: M = max max_s, sum = sum_s * exp(max_s - M).  No float atomics anywhere: the result depends on the row's bits, n and
// the split count, and the split count on (rows, n) only.
//
// Non-finite rows follow the float64 definition without a special case: a NaN entry gives exp(NaN); +inf gives inf - inf; a row
// of -inf only has max = -inf (reported as NaN at the end).  A PART that holds only -inf is legitimate (sum_s = 0), so a part
// subtracts 0 instead of a max of -inf, and its NaN entries still poison sum_s.
#include <cmath>
#include "ifa_host.h"
#include "ifa_device.h"

namespace ifa {

constexpr int LSE_THREADS = 256, LSE_WAVES = LSE_THREADS / 64, LSE_MAX_SPLITS = 64;

__device__ __forceinline__ float lse_block_max(float v, float *red, int tid)
{
    v = wave_max(v);
    __syncthreads();                    // (red is reused: the previous reduction's readers are done)
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ float lse_block_sum(float v, float *red, int tid)
{
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void lse_unpack(const uint4 &q, float *x)
{
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; e++) x[e] = hbits2f((uint16_t)((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu));
}

// lse of one (max, sum) pair -- the end of every path
__device__ __forceinline__ float lse_finish(float mx, float sum)
{
    if (mx == -INFINITY) return NAN;        // nothing but -inf: log(0) of the definition's NaN row
    return mx + logf(sum);                  // (NaN / +inf rows: sum is NaN already)
}

__device__ __forceinline__ float lse_target(const uint16_t *__restrict__ row, int n, const int *__restrict__ targets, int r)
{
    const int t = targets ? targets[r] : -1;
    return (t >= 0 && t < n) ? hbits2f(row[t]) : NAN;
}

// grid (splits, rows).  splits == 1: lse_out / target_out are written here; else part[(row * splits + split) * 2] = (max, sum).
__global__ void __launch_bounds__(LSE_THREADS) k_lse_rows(const uint16_t *__restrict__ logits, size_t row_stride, const int *__restrict__ row_idx, int n,
                                                          const int *__restrict__ targets, float *__restrict__ lse_out, float *__restrict__ target_out,
                                                          float *__restrict__ part)
{
    __shared__ float red[LSE_WAVES];
    const int tid = threadIdx.x, split = blockIdx.x, splits = gridDim.x, r = blockIdx.y;
    const size_t src_row = row_idx ? (size_t)row_idx[r] : (size_t)r;
    const uint16_t *row = logits + src_row * row_stride;
    // 16-byte loads over the aligned body, single halfs at the ragged ends (a row of an odd vocabulary starts at any 2-byte address)
    const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (n - head) >> 3;
    const int tail0 = head + (nvec << 3);
    const int per = (nvec + splits - 1) / splits;
    const int v0 = min(nvec, split * per), v1 = min(nvec, v0 + per);
    const uint4 *body = reinterpret_cast<const uint4 *>(row + head);
    // the ragged ends belong to the first / last part (fewer than 8 halfs each)
    float xe = -INFINITY; bool has_e = false;
    if (split == 0 && tid < head) { xe = hbits2f(row[tid]); has_e = true; }
    float xt = -INFINITY; bool has_t = false;
    if (split == splits - 1 && tail0 + tid < n) { xt = hbits2f(row[tail0 + tid]); has_t = true; }

    float mx = fmaxf(xe, xt);           // (fmaxf skips NaN: the sum pass meets it again)
    for (int v = v0 + tid; v < v1; v += LSE_THREADS) {
        float x[8];
        lse_unpack(body[v], x);
        mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7]))));
    }
    mx = lse_block_max(mx, red, tid);
    const float sub = mx == -INFINITY ? 0.0f : mx;

    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int v = v0 + tid; v < v1; v += LSE_THREADS) {
        float x[8];
        lse_unpack(body[v], x);
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] += expf(x[e] - sub);
    }
    if (has_e) acc[0] += expf(xe - sub);
    if (has_t) acc[1] += expf(xt - sub);
    float sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    sum = lse_block_sum(sum, red, tid);
    if (tid == 0) {
        if (splits == 1) {
            lse_out[r] = lse_finish(mx, sum);
            if (target_out) target_out[r] = lse_target(row, n, targets, r);
        } else {
            part[((size_t)r * splits + split) * 2] = mx;
            part[((size_t)r * splits + split) * 2 + 1] = sum;
        }
    }
}

// one wave per row: lane s holds part s (splits <= 64)
__global__ void __launch_bounds__(64) k_lse_combine(const float *__restrict__ part, int splits, const uint16_t *__restrict__ logits, size_t row_stride,
                                                    const int *__restrict__ row_idx, int n, const int *__restrict__ targets,
                                                    float *__restrict__ lse_out, float *__restrict__ target_out)
{
    const int lane = threadIdx.x, r = blockIdx.x;
    float mx = -INFINITY, sum = 0.0f;
    if (lane < splits) { mx = part[((size_t)r * splits + lane) * 2]; sum = part[((size_t)r * splits + lane) * 2 + 1]; }
    const float M = wave_max(mx);
    // a part of -inf only: 0 (or NaN) * exp(-inf) = 0 (or NaN); with M = -inf every part is one: the result is NaN below
    const float scaled = lane < splits ? sum * expf(mx - (M == -INFINITY ? 0.0f : M)) : 0.0f;
    const float total = wave_sum(scaled);
    if (lane == 0) {
        lse_out[r] = lse_finish(M, total);
        if (target_out) {
            const size_t src_row = row_idx ? (size_t)row_idx[r] : (size_t)r;
            target_out[r] = lse_target(logits + src_row * row_stride, n, targets, r);
        }
    }
}

// workgroups a row is split over: one for a prompt's many rows, up to 64 for the one or few rows of a decode step (about 128
// workgroups in flight; parts = ceil(vectors / 256) at most, so a part holds about one vector per lane or more -- 1 x 32000: 16
// parts of 250 vectors)
int lse_splits(size_t rows, size_t n)
{
    if (rows >= 64) return 1;
    const size_t by_rows = 128 / rows, by_len = (n / 8 + LSE_THREADS - 1) / LSE_THREADS;
    return (int)std::max<size_t>(1, std::min<size_t>(std::min(by_rows, by_len), LSE_MAX_SPLITS));
}

size_t lse_workspace_floats(size_t rows, size_t n) { const int s = lse_splits(rows, n); return s > 1 ? rows * (size_t)s * 2 : 0; }

// engine-internal: rows row_idx_dev[0 .. rows) (null: 0 .. rows - 1) of logits [.][row_stride]; part_dev holds lse_workspace_floats()
int lse_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, const int *targets_dev, float *lse_out,
             float *target_out, float *part_dev, hipStream_t s)
{
    const int splits = part_dev ? lse_splits(rows, n) : 1;
    k_lse_rows<<<dim3((unsigned)splits, (unsigned)rows), dim3(LSE_THREADS), 0, s>>>((const uint16_t *)logits, row_stride, row_idx_dev, (int)n, targets_dev,
                                                                                      lse_out, target_out, part_dev);
    IFA_LAUNCH_CHECK();
    if (splits > 1) {
        k_lse_combine<<<dim3((unsigned)rows), dim3(64), 0, s>>>(part_dev, splits, (const uint16_t *)logits, row_stride, row_idx_dev, (int)n, targets_dev,
                                                                lse_out, target_out);
        IFA_LAUNCH_CHECK();
    }
    return IFA_OK;
}

} // namespace ifa

extern "C" {

size_t ifa_logsumexp_workspace(size_t rows, size_t n)
{
    return rows && n ? ifa::lse_workspace_floats(rows, n) * sizeof(float) : 0;
}

int ifa_logsumexp_rows(const void *logits_f16, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, const int *targets_dev,
                       float *lse_out_dev, float *target_logit_out_dev, void *workspace_dev, ifa_stream stream)
{
    IFA_REQUIRE(logits_f16 && lse_out_dev, "ifa_logsumexp_rows: null pointer");
    IFA_REQUIRE(n > 0 && n < 0x7FFFFFFFu && row_stride >= n, "ifa_logsumexp_rows: n %zu, row stride %zu", n, row_stride);
    IFA_REQUIRE(rows > 0 && rows <= 65535, "ifa_logsumexp_rows: rows %zu", rows);
    IFA_REQUIRE(!target_logit_out_dev || targets_dev, "ifa_logsumexp_rows: target_logit_out_dev without targets_dev");
    return ifa::lse_rows(logits_f16, row_stride, row_idx_dev, rows, n, targets_dev, lse_out_dev, target_logit_out_dev, (float *)workspace_dev,
                         ifa_s(stream));
}

} // extern "C"
