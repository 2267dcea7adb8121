// ifa_device.h -- device-side helpers shared by all gfx950 kernels.
// wave64 only; no CUDA-compat paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ifa_dtype.h"      // DType, block_capacity, block_bytes, ax8_eligible

namespace ifa {

typedef _Float16 half_t;

// ---- fp16 helpers (RN conversions, like CUDA __float2half_rn) -------------
__device__ __forceinline__ float h2f(half_t h) { return (float)h; }
// The empty asm keeps the fp32 value opaque so the compiler cannot fold the
// producing fmul/fadd and the conversion into v_fma_mixlo_f16, which rounds
// once from the exact result; the reference rounds to fp32 first, then to fp16.
__device__ __forceinline__ half_t f2h(float f) { asm volatile("" : "+v"(f)); return (half_t)f; }
__device__ __forceinline__ float hbits2f(uint16_t b) { return (float)__builtin_bit_cast(half_t, b); }
// byte B of a word as a float: ONE v_cvt_f32_ubyteN (the compiler extracts the byte first and converts with ubyte0:
// two instructions per value, measured in the dequantising GEMM kernels where they are a fifth of the VALU stream)
template <int B>
__device__ __forceinline__ float ubyte_f32(uint32_t w)
{
    float f;
    if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(w));
    else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(w));
    else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(w));
    else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(w));
    return f;
}
__device__ __forceinline__ uint16_t f2hbits(float f) { return __builtin_bit_cast(uint16_t, f2h(f)); }

// ---- wave64 reductions -----------------------------------------------------
// DPP within 16-lane rows, ds_bpermute across rows.  All lanes get the result.
template <typename T>
__device__ __forceinline__ T dpp_xor1(T v) { return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false); }
template <typename T>
__device__ __forceinline__ T dpp_xor2(T v) { return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false); }
template <typename T>
__device__ __forceinline__ T dpp_half_mirror(T v) { return __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false); }
template <typename T>
__device__ __forceinline__ T dpp_mirror(T v) { return __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false); }

__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, dpp_xor1(v));
    v = fmaxf(v, dpp_xor2(v));
    v = fmaxf(v, dpp_half_mirror(v));
    v = fmaxf(v, dpp_mirror(v));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

// max over each aligned group of 32 lanes (a Q8_B32T2 block == 32 lanes)
__device__ __forceinline__ float half_wave_max(float v)
{
    v = fmaxf(v, dpp_xor1(v));
    v = fmaxf(v, dpp_xor2(v));
    v = fmaxf(v, dpp_half_mirror(v));
    v = fmaxf(v, dpp_mirror(v));
    v = fmaxf(v, __shfl_xor(v, 16));
    return v;
}

// sum over each aligned group of 32 lanes (exact: integers)
__device__ __forceinline__ int half_wave_sum_i32(int v)
{
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    v += __shfl_xor(v, 16);
    return v;
}

// 8 half x 8 half products accumulated in fp32 (products of halfs are exact in fp32)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8v_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float dot8_f16(u32x4_t w, u32x4_t x, float acc)
{
    const half8v_t wh = __builtin_bit_cast(half8v_t, w);
    const half8v_t xh = __builtin_bit_cast(half8v_t, x);
#pragma unroll
    for (int i = 0; i < 8; i++) acc = __builtin_fmaf((float)wh[i], (float)xh[i], acc);
    return acc;
}

__device__ __forceinline__ int sdot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }

__device__ __forceinline__ uint32_t ld_u32_unaligned2(const uint8_t *p)
{   // 2-byte aligned 32-bit read
    const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
    return (uint32_t)q[0] | ((uint32_t)q[1] << 16);
}

} // namespace ifa
