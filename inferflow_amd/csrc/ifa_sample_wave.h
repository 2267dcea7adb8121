// ifa_sample_wave.h -- the candidate pool in the registers of one wave and the draw of one row on it: the device side of
// csrc/ifa_sample_rule.h, shared by k_sample_pool (ifa_sample_pool.hip: one wave per independent row) and k_sample_verify
// (ifa_sample_verify.hip: one wave per row of a draft step, the generator state handed on from row to row).
//
// The at most 256 entries live in the registers of the wave: entry i is lane i & 63 of register i >> 6.  The exponentials and the
// divisions run over the lanes; the three order-dependent parts -- the sort, the sequential float sum and the cut, the double
// interval starts and the search -- run as scalar code of the whole wave (every index is wave-uniform) that addresses the entries
// with v_readlane and a lane-id select: no LDS, no dependent memory round trips.  The sort's pending ranges and the interval starts sit
// in lanes of further registers the same way.  Every loop is bounded by the pool length; nothing waits for another workgroup.
#pragma once
#include "ifa_device.h"
#include "ifa_sample_rule.h"

namespace ifa {

using namespace ifa_sr;

// ---- the pool in the registers of one wave.  Indices are wave-uniform; an index is reduced to 0..255 so that every access is
// defined whatever the caller computes.
__device__ __forceinline__ int sr_rd4(int v0, int v1, int v2, int v3, int i)
{
    const int l = i & 63;
    switch ((i >> 6) & 3) {
    case 0: return __builtin_amdgcn_readlane(v0, l);
    case 1: return __builtin_amdgcn_readlane(v1, l);
    case 2: return __builtin_amdgcn_readlane(v2, l);
    default: return __builtin_amdgcn_readlane(v3, l);
    }
}

// (a write is a compare of the lane id and a select: the value is wave-uniform, only the addressed lane takes it)
__device__ __forceinline__ void sr_wr4(int &v0, int &v1, int &v2, int &v3, int i, int x, int lane)
{
    const bool mine = lane == (i & 63);
    const int r = (i >> 6) & 3;
    v0 = (mine && r == 0) ? x : v0;
    v1 = (mine && r == 1) ? x : v1;
    v2 = (mine && r == 2) ? x : v2;
    v3 = (mine && r == 3) ? x : v3;
}

// R registers per array: 1 serves pools of up to 64 entries (the usual pool of 50) without the register select
template <int R> struct SrWavePool {
    int w0, w1, w2, w3, i0, i1, i2, i3;      // weights (float bits) and ids
    int lo0, lo1, lo2, lo3, hi0, hi1, hi2, hi3;      // interval starts (double halves)
    int stk, lane;
    __device__ __forceinline__ int rd(int v0, int v1, int v2, int v3, int i) const
    {
        if constexpr (R == 1) return __builtin_amdgcn_readlane(v0, i & 63);
        else return sr_rd4(v0, v1, v2, v3, i);
    }
    __device__ __forceinline__ void wr(int &v0, int &v1, int &v2, int &v3, int i, int x)
    {
        if constexpr (R == 1) v0 = lane == (i & 63) ? x : v0;
        else sr_wr4(v0, v1, v2, v3, i, x, lane);
    }
    __device__ __forceinline__ sr_item get(int i) const
    {
        sr_item r;
        r.w = __int_as_float(rd(w0, w1, w2, w3, i));
        r.id = rd(i0, i1, i2, i3, i);
        return r;
    }
    __device__ __forceinline__ void set(int i, sr_item v)
    {
        wr(w0, w1, w2, w3, i, __float_as_int(v.w));
        wr(i0, i1, i2, i3, i, v.id);
    }
    __device__ __forceinline__ int stk_get(int j) const { return __builtin_amdgcn_readlane(stk, j & 63); }
    __device__ __forceinline__ void stk_set(int j, int v) { stk = lane == (j & 63) ? v : stk; }
    __device__ __forceinline__ double base_get(int i) const
    {
        const unsigned lo = (unsigned)rd(lo0, lo1, lo2, lo3, i), hi = (unsigned)rd(hi0, hi1, hi2, hi3, i);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    __device__ __forceinline__ void base_set(int i, double v)
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        wr(lo0, lo1, lo2, lo3, i, (int)(unsigned)(b & 0xFFFFFFFFull));
        wr(hi0, hi1, hi2, hi3, i, (int)(unsigned)(b >> 32));
    }
};

__device__ __forceinline__ int sr_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float sr_unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// (a 64-bit value every lane holds alike, moved into scalar registers)
__device__ __forceinline__ uint64_t sr_uni64(unsigned long long v)
{
    return ((uint64_t)(unsigned)sr_uni((int)(unsigned)(v >> 32)) << 32) | (uint64_t)(unsigned)sr_uni((int)(unsigned)(v & 0xFFFFFFFFull));
}

// the drawn row: n entries (1 .. 64 R) of a sampled strategy at ids / vals + base, drawn with the generator state st (wave-uniform).
// Returns the state behind the draw (two steps on); ok = false: a NaN value (nothing is written, the state comes back as it was).
template <int R>
__device__ __forceinline__ uint64_t sample_row(int n, int lane, size_t base, const int *__restrict__ ids, const uint16_t *__restrict__ vals, int strategy,
                                               float temperature, float top_p, int max_k, float min_p, uint64_t st, float *__restrict__ weights_out,
                                               int &token, int &index, bool &ok)
{
    SrWavePool<R> a;
    a.w0 = a.w1 = a.w2 = a.w3 = a.i0 = a.i1 = a.i2 = a.i3 = 0;
    a.lo0 = a.lo1 = a.lo2 = a.lo3 = a.hi0 = a.hi1 = a.hi2 = a.hi3 = a.stk = 0; a.lane = lane;
    int wv[4] = {0, 0, 0, 0}, iv[4] = {0, 0, 0, 0};
    bool has_nan = false, unordered = false;      // unordered: an entry that is not above its successor (equal values): the sort has something to decide
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int i = r * 64 + lane;
        float w = 0.0f; int id = 0;
        if (i < n) { w = sr_half_bits_to_float(vals[base + i]); id = ids[base + i]; }
        if (i + 1 < n) unordered = unordered || !(w > sr_half_bits_to_float(vals[base + i + 1]));
        has_nan = has_nan || w != w;
        wv[r] = __float_as_int(w); iv[r] = id;
    }
    a.w0 = wv[0]; a.w1 = wv[1]; a.w2 = wv[2]; a.w3 = wv[3];
    a.i0 = iv[0]; a.i1 = iv[1]; a.i2 = iv[2]; a.i3 = iv[3];
    ok = __ballot(has_nan) == 0ull;
    if (!ok) return st;
    if (__ballot(unordered) != 0ull) sr_sort_unordered(a, n);      // (sr_sort's own test, taken over the lanes)
    // (sorted and free of NaN: the maximum SoftMaxPool looks for is the first weight)
    const float m = a.get(0).w, t = sr_temperature(temperature);
    wv[0] = a.w0; wv[1] = a.w1; wv[2] = a.w2; wv[3] = a.w3;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r * 64 + lane < n) wv[r] = __float_as_int(sr_exp(__int_as_float(wv[r]), m, t));
    a.w0 = wv[0]; a.w1 = wv[1]; a.w2 = wv[2]; a.w3 = wv[3];
    const float sum = sr_sum(a, n);
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r * 64 + lane < n) {
            const float p = __int_as_float(wv[r]) / sum;
            wv[r] = __float_as_int(p);
            if (weights_out) weights_out[base + r * 64 + lane] = p;
        }
    a.w0 = wv[0]; a.w1 = wv[1]; a.w2 = wv[2]; a.w3 = wv[3];
    const int len = sr_cut(a, n, strategy, top_p, max_k, min_p);
    index = sr_draw(a, len, st);
    token = a.get(index).id;
    return st;
}

} // namespace ifa
