// ifa_dtype.h -- element type ids and block geometry: plain constexpr functions, no HIP header, so that the pure host plans
// (ifa_decode_gemv_plan.h) and the kernels read ONE definition.  ifa_device.h includes it for every kernel.
#pragma once

#ifdef __HIPCC__
#define IFA_HD __host__ __device__
#else
#define IFA_HD
#endif

namespace ifa {

// dtype ids == reference ElementType enum (src/tensor/tensor_common.h:15-42)
enum DType : int {
    F32 = 0, F16 = 1,
    Q8_B32T1 = 7, Q8_B32T2 = 8, Q6_B64T1 = 9, Q5_B64T1 = 10, Q5_B32T1 = 11,
    Q4_B16 = 12, Q4_B32T1A = 13, Q4_B32T1B = 14, Q4_B64T1 = 17, Q3H_B64T1 = 18,
    Q3_B32T1A = 19, Q3_B32T1B = 20, Q2_B32T1A = 21, Q2_B32T1B = 22
};

// internal id (no tensor of the C ABI has it; ifa_decode_gemv_plan accepts it as a format to plan for, and ifa_model_gemv_plan reports it):
// Q3H_B64T1 values streamed at their native 32 bytes per block by the fused decode GEMV
// (ifa_decode_formats.h WRowQ3HN; engine option q3h_native) instead of the 36-byte nibble-pair form
constexpr int Q3H_NATIVE = 99;

IFA_HD constexpr int block_capacity(int dt)
{
    return (dt == F32 || dt == F16) ? 1
        : (dt == Q4_B16) ? 16
        : (dt == Q6_B64T1 || dt == Q5_B64T1 || dt == Q4_B64T1 || dt == Q3H_B64T1 || dt == Q3H_NATIVE) ? 64
        : (dt == Q8_B32T1 || dt == Q8_B32T2 || dt == Q5_B32T1 || dt == Q4_B32T1A || dt == Q4_B32T1B
           || dt == Q3_B32T1A || dt == Q3_B32T1B || dt == Q2_B32T1A || dt == Q2_B32T1B) ? 32 : 0;
}

IFA_HD constexpr int block_bytes(int dt)
{
    return dt == F32 ? 4 : dt == F16 ? 2
        : dt == Q8_B32T1 ? 36 : dt == Q8_B32T2 ? 34 : dt == Q6_B64T1 ? 52 : dt == Q5_B64T1 ? 44
        : dt == Q5_B32T1 ? 24 : dt == Q4_B16 ? 10 : (dt == Q4_B32T1A || dt == Q4_B32T1B) ? 20
        : dt == Q4_B64T1 ? 36 : (dt == Q3H_B64T1 || dt == Q3H_NATIVE) ? 32 : (dt == Q3_B32T1A || dt == Q3_B32T1B) ? 16
        : (dt == Q2_B32T1A || dt == Q2_B32T1B) ? 12 : 0;
}

IFA_HD constexpr bool ax8_eligible(int dt)
{   // GetUseFullQuantGemv, src/transformer/inference_worker.cc:2707-2730
    return dt == Q8_B32T2 || dt == Q6_B64T1 || dt == Q5_B64T1 || dt == Q4_B32T1A || dt == Q4_B32T1B
        || dt == Q4_B64T1 || dt == Q3H_B64T1;
}

} // namespace ifa
