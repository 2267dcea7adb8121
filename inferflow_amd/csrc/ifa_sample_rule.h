// ifa_sample_rule.h -- the draw of the sampled strategies, written once for the host and the device: what
// ChooseTokensFromPool (host/sampling_strategy.cc) does behind the candidate pool for sample.std (1), greedy (2), top_k (3),
// sample.top_p (4) and min_p (7) -- std::sort of the pool, SoftMaxPool, the strategy's cut, DrawOne with the 48-bit LCG of
// java.util.Random.  Every step is spelled out (no std:: algorithm, no std::max whose NaN behaviour is implicit); the sort is
// libstdc++'s std::sort restated (oracle/sampling.py:std_sort is its specification): it is NOT stable, so the order of EQUAL
// F16 logits -- common in a pool -- is this algorithm's doing and decides which id a draw returns.
//
// The code reads and writes the pool through an accessor A, so that the host keeps it in arrays and the kernel in the registers
// of one wave (csrc/ifa_sample_pool.hip):
//   sr_item get(int i) / void set(int i, sr_item)     entry i of the pool (weight, id)
//   int stk_get(int j) / void stk_set(int j, int v)   SR_STACK words for the sort's pending ranges
//   double base_get(int i) / void base_set(int i, double)   the draw's interval starts
// Everything except the exponential is integer or correctly rounded IEEE arithmetic (the build sets -ffp-contract=off and no
// fast-math flag); exp is the platform's double exp -- glibc's on the host, ocml's (1 ulp) on the device -- rounded to float.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IFA_SR_HD __host__ __device__ __forceinline__
#else
#define IFA_SR_HD inline
#endif

namespace ifa_sr {

struct sr_item { float w; int id; };

constexpr int SR_MAX = 256;        // IFA_POOL_MAX
constexpr int SR_STACK = 24;       // pending ranges of the introsort: at most its depth limit, 2 * floor(log2 256) = 16
constexpr int SR_SORT_RUN = 16;    // libstdc++'s _S_threshold

enum { SR_STD = 1, SR_GREEDY = 2, SR_TOP_K = 3, SR_TOP_P = 4, SR_MIN_P = 7 };

IFA_SR_HD bool sr_strategy_ok(int id) { return id == SR_STD || id == SR_GREEDY || id == SR_TOP_K || id == SR_TOP_P || id == SR_MIN_P; }

// ---- java.util.Random (sslib::Random): seed' = (seed * 0x5DEECE66D + 0xB) mod 2^48; the state is the scrambled seed
IFA_SR_HD int32_t sr_next(uint64_t &state, int bits)
{
    state = (state * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1ULL);
    return (int32_t)(state >> (48 - bits));
}

IFA_SR_HD double sr_next_double(uint64_t &state)
{
    const int64_t hi = (int64_t)sr_next(state, 26) << 27;
    const int64_t lo = (int64_t)sr_next(state, 27);
    return (double)(hi + lo) / 9007199254740992.0;      // 2^53: exact
}

// ---- std::sort(first, last, [](a, b) { return a.weight > b.weight; })
IFA_SR_HD bool sr_less(const sr_item &a, const sr_item &b) { return a.w > b.w; }

template <class A> IFA_SR_HD void sr_swap(A &a, int i, int j)
{
    const sr_item x = a.get(i), y = a.get(j);
    a.set(i, y); a.set(j, x);
}

template <class A> IFA_SR_HD void sr_move_median_to_first(A &a, int result, int x, int y, int z)
{
    const sr_item ix = a.get(x), iy = a.get(y), iz = a.get(z);
    if (sr_less(ix, iy)) {
        if (sr_less(iy, iz)) sr_swap(a, result, y);
        else if (sr_less(ix, iz)) sr_swap(a, result, z);
        else sr_swap(a, result, x);
    } else if (sr_less(ix, iz)) sr_swap(a, result, x);
    else if (sr_less(iy, iz)) sr_swap(a, result, z);
    else sr_swap(a, result, y);
}

template <class A> IFA_SR_HD int sr_unguarded_partition(A &a, int first, int last, int pivot)
{
    // (the bounds hi / pivot never stop a scan under a strict weak order -- the median sits at the pivot -- they only make every
    // loop finite whatever the weights are)
    const int hi = last;
    for (;;) {
        const sr_item p = a.get(pivot);
        while (first < hi && sr_less(a.get(first), p)) first++;
        last--;
        while (last > pivot && sr_less(p, a.get(last))) last--;
        if (!(first < last)) return first;
        sr_swap(a, first, last);
        first++;
    }
}

// std::__adjust_heap over [first, first + length)
template <class A> IFA_SR_HD void sr_adjust_heap(A &a, int first, int hole, int length, sr_item val)
{
    const int top = hole;
    int child = hole;
    while (child < (length - 1) / 2) {
        child = 2 * (child + 1);
        if (sr_less(a.get(first + child), a.get(first + child - 1))) child--;
        a.set(first + hole, a.get(first + child));
        hole = child;
    }
    if ((length & 1) == 0 && child == (length - 2) / 2) {
        child = 2 * (child + 1);
        a.set(first + hole, a.get(first + child - 1));
        hole = child - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && sr_less(a.get(first + parent), val)) {
        a.set(first + hole, a.get(first + parent));
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a.set(first + hole, val);
}

// std::partial_sort(first, last, last): make_heap + sort_heap
template <class A> IFA_SR_HD void sr_heap_sort(A &a, int first, int last)
{
    const int length = last - first;
    if (length >= 2)
        for (int parent = (length - 2) / 2;; parent--) {
            sr_adjust_heap(a, first, parent, length, a.get(first + parent));
            if (parent == 0) break;
        }
    while (last - first > 1) {
        last--;
        const sr_item val = a.get(last);
        a.set(last, a.get(first));
        sr_adjust_heap(a, first, 0, last - first, val);
    }
}

template <class A> IFA_SR_HD void sr_unguarded_linear_insert(A &a, int i)
{
    const sr_item val = a.get(i);
    int nxt = i - 1;
    while (nxt >= 0 && sr_less(val, a.get(nxt))) {      // (nxt >= 0: never the stop under a strict weak order)
        a.set(i, a.get(nxt));
        i = nxt;
        nxt--;
    }
    a.set(i, val);
}

template <class A> IFA_SR_HD void sr_insertion_sort(A &a, int first, int last)
{
    for (int i = first + 1; i < last; i++) {
        const sr_item val = a.get(i);
        if (sr_less(val, a.get(first))) {
            for (int j = i; j > first; j--) a.set(j, a.get(j - 1));      // move_backward
            a.set(first, val);
        } else sr_unguarded_linear_insert(a, i);
    }
}

// The introsort loop recurses into the right part and goes on with the left one; the two ranges are disjoint, so the right part
// waits on a stack instead (at most one pending range per level of the depth limit) and the result is the same.
template <class A> IFA_SR_HD void sr_sort_unordered(A &a, int n)
{
    if (n < 2) return;
    int lg = 0;
    while ((n >> (lg + 1)) != 0) lg++;
    int sp = 0;
    a.stk_set(sp++, (0 << 16) | (n << 5) | (2 * lg));      // first (9 bits) | last (11 bits) | depth (5 bits)
    while (sp > 0) {
        const int e = a.stk_get(--sp);
        const int first = e >> 16;
        int last = (e >> 5) & 0x7FF, depth = e & 31;
        while (last - first > SR_SORT_RUN) {
            if (depth == 0) { sr_heap_sort(a, first, last); break; }
            depth--;
            const int mid = first + (last - first) / 2;
            sr_move_median_to_first(a, first, first + 1, mid, last - 1);
            const int cut = sr_unguarded_partition(a, first + 1, last, first);
            if (sp < SR_STACK) a.stk_set(sp++, (cut << 16) | (last << 5) | depth);
            last = cut;
        }
    }
    if (n > SR_SORT_RUN) {
        sr_insertion_sort(a, 0, SR_SORT_RUN);
        for (int i = SR_SORT_RUN; i < n; i++) sr_unguarded_linear_insert(a, i);
    } else sr_insertion_sort(a, 0, n);
}

// the sort is the identity where the pool is strictly descending (no equal neighbours, no NaN): nothing to decide
template <class A> IFA_SR_HD bool sr_strictly_descending(A &a, int n)
{
    float prev = a.get(0).w;
    for (int i = 1; i < n; i++) {
        const float w = a.get(i).w;
        if (!(prev > w)) return false;
        prev = w;
    }
    return true;
}

template <class A> IFA_SR_HD void sr_sort(A &a, int n)
{
    if (n < 2 || sr_strictly_descending(a, n)) return;
    sr_sort_unordered(a, n);
}

// ---- SoftMaxPool, in its parts: the maximum, e = (float)exp((double)((w - max) / t)), the sequential float sum, p = e / sum
IFA_SR_HD float sr_temperature(float t) { return t < 0.001f ? 0.001f : t; }

template <class A> IFA_SR_HD float sr_max(A &a, int n)
{
    float m = a.get(0).w;
    for (int i = 0; i < n; i++) {      // std::max(m, w) = m < w ? w : m
        const float w = a.get(i).w;
        m = m < w ? w : m;
    }
    return m;
}

IFA_SR_HD float sr_exp(float w, float m, float t) { return (float)::exp((double)((w - m) / t)); }

template <class A> IFA_SR_HD float sr_sum(A &a, int n)
{
    float sum = 0;
    for (int i = 0; i < n; i++) sum += a.get(i).w;
    if (sum < 0.00001f) sum = 0.00001f;
    return sum;
}

// ---- the cut on the sorted, softmaxed pool: how many leading entries the draw sees
template <class A> IFA_SR_HD int sr_cut(A &a, int n, int strategy, float top_p_cfg, int max_k, float min_p)
{
    if (strategy == SR_MIN_P) {                                  // CutMinP
        const float scale = a.get(0).w;
        int len = 1;
        for (int i = 1; i < n; i++) {
            if (a.get(i).w < min_p * scale) break;
            len++;
        }
        return len;
    }
    const float top_p = (strategy == SR_STD || strategy == SR_TOP_P) ? top_p_cfg : 1.0f;
    const int top_k = n < max_k ? n : max_k;                     // std::min(n, max_k)
    float cumulative = 0;
    int len = 0;
    for (int i = 0; i < n; i++) {                                // topp_topk_filter_on_sorted
        cumulative += a.get(i).w;
        len++;
        if (cumulative >= top_p || len >= top_k) break;
    }
    return len;
}

// ---- DrawOne over the first `len` entries: the index of the chosen one; advances the generator by two steps
template <class A> IFA_SR_HD int sr_draw(A &a, int len, uint64_t &rng)
{
    double upper = 0;
    for (int i = 0; i < len; i++) {
        a.base_set(i, upper);
        const double p = (double)a.get(i).w;
        upper += 0.0 < p ? p : 0.0;                              // std::max(0.0, p): a NaN counts as 0
    }
    const double r = 0.0 + sr_next_double(rng) * (upper - 0.0);  // NextDouble(0, upper)
    // the reference's interval search, including its behaviour at the interval ends
    uint32_t begin = 0, end = (uint32_t)len - 1, mid = begin;
    while (begin < end) {
        mid = (end + begin) / 2;
        if (r < a.base_get((int)mid)) end = mid;
        else if (r > a.base_get((int)mid + 1)) { begin = mid + 1; mid = begin; }
        else break;
    }
    return (int)mid;
}

// F16 bits -> float, exactly (host/half_bits.h restated for both sides)
IFA_SR_HD float sr_half_bits_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t ex = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
    if (ex == 0) {
        if (man == 0) bits = sign;
        else {
            int e = -1;
            do { man <<= 1; e++; } while (!(man & 0x400u));
            bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13);
        }
    } else if (ex == 31) bits = sign | 0x7f800000u | (man << 13);
    else bits = sign | ((ex + 112u) << 23) | (man << 13);
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

} // namespace ifa_sr
