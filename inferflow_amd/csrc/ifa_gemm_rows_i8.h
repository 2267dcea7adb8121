// ifa_gemm_rows_i8.h -- launch interface of k_gemm_rows_i8 (ifa_gemm_rows_i8.hip): the 2..32-row weight-streaming GEMM over tiled
// Q4_B32T1 weights on v_mfma_i32_16x16x32_i8, every output row bit-equal to the decode GEMV of that row (docs/rows_gemm_int8.md).
#pragma once
#include "ifa_gemm_rows_mfma.h"
#include "ifa_gemm_rows_i8_plan.h"

namespace ifa {

// the facts of a launch: P.Wt[] / P.Wt1 are the tiled rows, everything else as for k_gemm_rows_mfma
GemmRowsI8Facts gemm_rows_i8_facts(int w_dtype, const GmArgs &P, int epi, int norm);
// the plan does not refuse the launch
bool gemm_rows_i8_ok(int w_dtype, const GmArgs &P, int epi, int norm);
// num_cus > 0: plan for that many CUs instead of the device's (tests: more tiles per workgroup at small shapes)
int gemm_rows_i8_launch(int w_dtype, const GmArgs &P, int epi, int norm, hipStream_t s, int num_cus = 0);

} // namespace ifa
