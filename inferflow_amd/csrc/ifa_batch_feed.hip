// ifa_batch_feed.hip -- the feed rule of csrc/ifa_batch_feed.h on the device: one launch behind a batched decode step picks the
// token of each of the n rows, freezes a row at its stop id, appends to the token ring and advances token, position and the
// context of every layer's attention row, so that the next replay of the step needs nothing from the host.  The same header
// compiled for the host is ifa_batch_feed_host, the reference the tests compare the kernel with bit for bit.
//
// One workgroup.  Everything that more than one row shares -- the step counter, the error word -- is read in front of the
// one barrier and written behind it by thread 0, and what a row owns is written by the row's thread, so there is no atomic and no
// order between workgroups to rely on.  The layers x n attention entries (80 x 32 at most for the models of the README) are
// spread over the workgroup's threads, up to 1024 of them: two or three independent read-modify-writes per thread.
#include <algorithm>
#include "ifa_engine_state.h"
#include "ifa_batch_feed.h"

namespace ifa {

using namespace ifa_bf;

static_assert(sizeof(AttnRowH) == sizeof(bf_attn_row) && offsetof(AttnRowH, n_ctx) == offsetof(bf_attn_row, n_ctx),
              "bf_attn_row restates the batched step's AttnRowH");

__global__ void __launch_bounds__(1024) k_batch_feed(const ifa_batch_feed_args a)
{
    __shared__ int flags[IFA_BATCH_ROWS_MAX];
    const int tid = (int)threadIdx.x, n = a.n;
    const int s = *a.step;
    const bool ok = bf_step_ok(a, s);
    if (tid < n) flags[tid] = ok ? bf_feed_row(a, s, tid) : 0;
    __syncthreads();
    if (tid == 0) {
        if (!ok) { if (*a.err == 0) *a.err = -1; }
        else {
            for (int r = 0; r < n; r++)
                if ((flags[r] & BF_FAIL) && *a.err == 0) { *a.err = bf_err_code(a, s, r); break; }
            *a.step = s + 1;
        }
    }
    bf_attn_row *rows = (bf_attn_row *)a.attn_rows;
    const int entries = a.layers * n;
    for (int i = tid; i < entries; i += (int)blockDim.x)
        if (flags[i % n] & BF_ADVANCE) rows[i].n_ctx = rows[i].n_ctx + 1;
}

// counts[r] = min(counts[r], pool_len[r]): the pool of a step is built with the step's one k; a row draws from its own length
__global__ void __launch_bounds__(64) k_batch_clamp_counts(int *__restrict__ counts, const int *__restrict__ pool_len, int rows)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r < rows) counts[r] = min(counts[r], pool_len[r]);
}

static int feed_args_check(const ifa_batch_feed_args *a, const char *who)
{
    IFA_REQUIRE(a && a->struct_size == (int)sizeof(ifa_batch_feed_args), "%s: struct_size is not %zu", who, sizeof(ifa_batch_feed_args));
    IFA_REQUIRE(a->n >= 1 && a->n <= IFA_BATCH_ROWS_MAX, "%s: n %d outside 1..%d", who, a->n, IFA_BATCH_ROWS_MAX);
    IFA_REQUIRE(a->layers >= 0 && a->layers <= IFA_BATCH_LAYERS_MAX, "%s: layers %d outside 0..%d", who, a->layers, IFA_BATCH_LAYERS_MAX);
    IFA_REQUIRE(a->ring_steps >= 1 && a->ring_steps <= IFA_BATCH_STEPS_MAX, "%s: ring_steps %d outside 1..%d", who, a->ring_steps, IFA_BATCH_STEPS_MAX);
    IFA_REQUIRE(a->rows && a->step && a->tok && a->pos && a->ring && a->pair_slot && a->pair_tok && a->err, "%s: null pointer", who);
    IFA_REQUIRE(a->layers == 0 || a->attn_rows, "%s: %d layers without an attention table", who, a->layers);
    IFA_REQUIRE((a->pool_ids == nullptr) == (a->pool_counts == nullptr), "%s: pool_ids and pool_counts come together", who);
    IFA_REQUIRE(!a->pool_ids || (a->k_stride >= 1 && a->k_stride <= IFA_POOL_MAX), "%s: k_stride %d outside 1..%d", who, a->k_stride, IFA_POOL_MAX);
    return IFA_OK;
}

} // namespace ifa

extern "C" {

int ifa_batch_feed_rows(const ifa_batch_feed_args *args_dev_arrays, ifa_stream stream)
{
    const ifa_batch_feed_args *a = args_dev_arrays;
    int rc = ifa::feed_args_check(a, "ifa_batch_feed_rows");
    if (rc) return rc;
    const int entries = a->layers * a->n;
    const unsigned threads = (unsigned)std::min(1024, std::max(64, (entries + 63) / 64 * 64));
    ifa::k_batch_feed<<<dim3(1), dim3(threads), 0, ifa_s(stream)>>>(*a);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// host-only: the same rule on the CPU
int ifa_batch_feed_host(const ifa_batch_feed_args *a)
{
    using namespace ifa_bf;
    int rc = ifa::feed_args_check(a, "ifa_batch_feed_host");
    if (rc) return rc;
    const int s = *a->step;
    if (!bf_step_ok(*a, s)) { if (*a->err == 0) *a->err = -1; return IFA_OK; }
    bf_attn_row *rows = (bf_attn_row *)a->attn_rows;
    for (int r = 0; r < a->n; r++) {
        const int f = bf_feed_row(*a, s, r);
        if ((f & BF_FAIL) && *a->err == 0) *a->err = bf_err_code(*a, s, r);
        if (f & BF_ADVANCE)
            for (int l = 0; l < a->layers; l++) rows[(size_t)l * (size_t)a->n + r].n_ctx += 1;
    }
    *a->step = s + 1;
    return IFA_OK;
}

int ifa_batch_clamp_counts(int *counts_dev, const int *pool_len_dev, size_t rows, ifa_stream stream)
{
    IFA_REQUIRE(counts_dev && pool_len_dev, "ifa_batch_clamp_counts: null pointer");
    IFA_REQUIRE(rows > 0 && rows <= 65535, "ifa_batch_clamp_counts: rows %zu", rows);
    ifa::k_batch_clamp_counts<<<dim3(ifa_cdiv(rows, 64)), dim3(64), 0, ifa_s(stream)>>>(counts_dev, pool_len_dev, (int)rows);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // extern "C"
