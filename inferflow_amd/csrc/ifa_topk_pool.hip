// ifa_topk_pool.hip -- the candidate pool of the sampling strategies on the device: SamplingStrategy::GetSortedTopK
// (src/transformer/sampling_strategy.cc:281-297; host/sampling_strategy.cc SortedTopK) over F16 logits rows.  The result is
// defined by a total order -- higher value first, lower id among equal values, NaN and the masked ids never offered -- so it
// equals the host function's element for element.
//
// One workgroup of 1024 threads per row; the row (64 KB at 32000 ids, 300 KB at 150K) sits in L2 behind the lm_head launch, so
// this is a latency problem.  Every F16 maps to a monotone 16-bit key (+0.0 and -0.0 collapse to one key: they are the same
// float).  The k-th key is found by radix select -- a 256-bin LDS histogram of the high byte, then of the low byte inside
// the chosen bin -- the entries above it and the lowest-id ties at it are compacted into LDS as (key << 32) | (0xFFFFFFFF - id)
// words (the packing of argmax_scan's keys in ifa_decode_lmhead_tail.h: an unsigned maximum is the best entry) and a bitonic
// network sorts the at most 256 words.  Ties at the threshold need id order only when there are more of them than wanted; then
// every wave walks a contiguous range of ids and ranks its ties with ballots.
#include "ifa_host.h"
#include "ifa_device.h"

namespace ifa {

constexpr int POOL_THREADS = 1024, POOL_WAVES = POOL_THREADS / 64;

// 0 = not offered (NaN); else 0x03FF (-inf) .. 0xFC00 (+inf), both zeros 0x8000
__device__ __forceinline__ unsigned pool_key(unsigned h)
{
    const unsigned mag = h & 0x7FFFu;
    if (mag > 0x7C00u) return 0u;
    if (mag == 0u) return 0x8000u;
    return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}

__device__ __forceinline__ bool pool_masked(const unsigned *__restrict__ excl, int id)
{
    return excl && ((excl[id >> 5] >> (id & 31)) & 1u);
}

// f(id, key) for every offered entry of the row: 16-byte loads over the aligned body, single halfs at the ragged ends (a row of
// an odd vocabulary starts at any 2-byte address)
template <typename F>
__device__ __forceinline__ void pool_scan(const uint16_t *__restrict__ row, int n, const unsigned *__restrict__ excl, int tid, F f)
{
    const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (n - head) >> 3;
    if (tid < head) {
        const unsigned key = pool_key(row[tid]);
        if (key && !pool_masked(excl, tid)) f(tid, key);
    }
    const uint4 *body = reinterpret_cast<const uint4 *>(row + head);
    for (int v = tid; v < nvec; v += POOL_THREADS) {
        const uint4 q = body[v];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        const int id0 = head + (v << 3);
        unsigned m0 = 0u, m1 = 0u;
        if (excl) { m0 = excl[id0 >> 5]; m1 = excl[(id0 + 7) >> 5]; }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int id = id0 + e;
            const unsigned key = pool_key((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
            const unsigned mw = ((id >> 5) == (id0 >> 5)) ? m0 : m1;
            if (key && !((mw >> (id & 31)) & 1u)) f(id, key);
        }
    }
    const int tail = head + (nvec << 3) + tid;
    if (tail < n) {
        const unsigned key = pool_key(row[tail]);
        if (key && !pool_masked(excl, tail)) f(tail, key);
    }
}

// the bin of a 256-bin histogram that holds the want-th entry from the top: sel[0] = bin, sel[1] = entries above it
// (threads 0..255; sel[0] stays -1 if the histogram holds fewer than `want`)
__device__ __forceinline__ void pool_pick_bin(const unsigned *hist, int want, int tid, int *sel)
{
    if (tid < 256) {
        unsigned above = 0;
        for (int j = tid + 1; j < 256; j++) above += hist[j];
        if ((int)above < want && (int)(above + hist[tid]) >= want) { sel[0] = tid; sel[1] = (int)above; }
    }
}

__global__ void __launch_bounds__(POOL_THREADS) k_topk_pool(const uint16_t *__restrict__ logits, size_t row_stride, const int *__restrict__ row_idx, int n, int k,
                                                            const unsigned *__restrict__ excl, int *__restrict__ ids_out,
                                                            uint16_t *__restrict__ vals_out, int *__restrict__ count_out)
{
    __shared__ unsigned hist1[256], hist2[256];
    __shared__ unsigned long long list[IFA_POOL_MAX];
    __shared__ int sel1[2], sel2[2], wave_ties[POOL_WAVES];
    __shared__ unsigned n_list, total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t src_row = row_idx ? (size_t)row_idx[blockIdx.x] : (size_t)blockIdx.x;
    const uint16_t *row = logits + src_row * row_stride;
    if (tid < 256) { hist1[tid] = 0u; hist2[tid] = 0u; list[tid] = 0ull; }
    if (tid == 0) { sel1[0] = -1; sel1[1] = 0; sel2[0] = -1; sel2[1] = 0; n_list = 0u; total = 0u; }
    __syncthreads();
    // ---- pass 1: high byte of every offered key
    pool_scan(row, n, excl, tid, [&](int, unsigned key) { atomicAdd(&hist1[key >> 8], 1u); });
    __syncthreads();
    pool_pick_bin(hist1, k, tid, sel1);
    if (tid == 0) { unsigned t = 0; for (int j = 0; j < 256; j++) t += hist1[j]; total = t; }
    __syncthreads();
    const int offered = (int)total;
    const bool take_all = offered <= k;                     // a short pool: every offered entry, no threshold
    const int cnt = take_all ? offered : k;
    unsigned thr = 0u;                                      // keys above thr are in; `need` of the `ties` keys equal to it too
    int G = 0, need = 0, ties = 0;
    if (!take_all) {
        const unsigned b1 = (unsigned)max(sel1[0], 0);
        // ---- pass 2: low byte inside the bin of the k-th key
        pool_scan(row, n, excl, tid, [&](int, unsigned key) { if ((key >> 8) == b1) atomicAdd(&hist2[key & 255u], 1u); });
        __syncthreads();
        pool_pick_bin(hist2, k - sel1[1], tid, sel2);
        __syncthreads();
        const int b2 = max(sel2[0], 0);
        thr = (b1 << 8) | (unsigned)b2;
        G = sel1[1] + sel2[1];
        need = k - G;
        ties = (int)hist2[b2];
    }
    // ---- pass 3: compaction.  Order inside the list does not matter (it is sorted below) unless only some of the ties enter
    const bool ordered_ties = !take_all && ties > need;
    pool_scan(row, n, excl, tid, [&](int id, unsigned key) {
        if (take_all || key > thr || (key == thr && !ordered_ties)) {
            const unsigned slot = atomicAdd(&n_list, 1u);
            if (slot < (unsigned)IFA_POOL_MAX) list[slot] = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)id);
        }
    });
    if (ordered_ties) {
        // the `need` lowest ids among the ties: wave w owns ids [w * seg, (w + 1) * seg), counts its ties, then ranks them in id order
        const int seg = (((n + POOL_WAVES - 1) / POOL_WAVES) + 63) & ~63;
        const int lo = wave * seg, hi = min(n, lo + seg);
        int c = 0;
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int id = i0 + lane;
            const bool tie = id < hi && pool_key(row[id]) == thr && !pool_masked(excl, id);
            c += __popcll(__ballot(tie));
        }
        if (lane == 0) wave_ties[wave] = c;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; w++) before += wave_ties[w];
        for (int i0 = lo; i0 < hi && before < need; i0 += 64) {
            const int id = i0 + lane;
            const bool tie = id < hi && pool_key(row[id]) == thr && !pool_masked(excl, id);
            const unsigned long long mask = __ballot(tie);
            const int rank = before + __popcll(mask & ((1ull << lane) - 1ull));
            if (tie && rank < need && G + rank < IFA_POOL_MAX)
                list[G + rank] = ((unsigned long long)thr << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)id);
            before += __popcll(mask);
        }
    }
    __syncthreads();
    // ---- bitonic sort, descending, over the next power of two (the unused slots hold 0: below every key)
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < (P >> 1)) {
                const int pos = 2 * tid - (tid & (stride - 1)), other = pos + stride;
                const unsigned long long a = list[pos], b = list[other];
                if ((a < b) == ((pos & size) == 0)) { list[pos] = b; list[other] = a; }
            }
            __syncthreads();
        }
    if (tid < cnt) {
        const int id = (int)(0xFFFFFFFFu - (unsigned)(list[tid] & 0xFFFFFFFFull));
        ids_out[(size_t)blockIdx.x * k + tid] = id;
        vals_out[(size_t)blockIdx.x * k + tid] = row[min(max(id, 0), n - 1)];
    }
    if (tid == 0) count_out[blockIdx.x] = cnt;
}

// engine-internal: the pool of rows row_idx_dev[0 .. rows) (null: rows 0 .. rows - 1) of logits [.][row_stride]
int topk_pool_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, int k, const unsigned *excl,
                   int *ids_out, void *vals_out, int *count_out, hipStream_t s)
{
    k_topk_pool<<<dim3((unsigned)rows), dim3(POOL_THREADS), 0, s>>>((const uint16_t *)logits, row_stride, row_idx_dev, (int)n, k, excl, ids_out,
                                                                   (uint16_t *)vals_out, count_out);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

} // namespace ifa

extern "C" {

int ifa_topk_pool(const void *logits_f16, size_t rows, size_t n, int k, const unsigned *excluded_bits_dev,
                  int *ids_out_dev, void *vals_out_f16_dev, int *count_out_dev, ifa_stream stream)
{
    IFA_REQUIRE(logits_f16 && ids_out_dev && vals_out_f16_dev && count_out_dev, "ifa_topk_pool: null pointer");
    IFA_REQUIRE(k >= 1 && k <= IFA_POOL_MAX, "ifa_topk_pool: k %d outside 1..%d", k, IFA_POOL_MAX);
    IFA_REQUIRE(n > 0 && n < 0x7FFFFFFFu, "ifa_topk_pool: n %zu", n);
    IFA_REQUIRE(rows > 0 && rows <= 65535, "ifa_topk_pool: rows %zu", rows);
    return ifa::topk_pool_rows(logits_f16, n, nullptr, rows, n, k, excluded_bits_dev, ids_out_dev, vals_out_f16_dev, count_out_dev, ifa_s(stream));
}

} // extern "C"
