// ifa_decode_gemv_impl.h -- included by exactly one ifa_dgemv_<format>.hip per format.
#pragma once
#include <algorithm>
#include "ifa_decode_gemv.h"

namespace ifa {

// (the tuning overrides IFA_T_* and dec_role / dec_rw / dec_threads / dec_np: ifa_decode_gemv_plan.h)

// The run-time values of a launch -- blocks per lane, chunks, grid, LDS bytes -- come from the plan (plan_dec_gemv); the template
// arguments of the instance from the same dec_rw / dec_threads / dec_np the plan called, for the plan's nj / njl.
template <int DT, int EPI, int NORM, bool XADD = false>
static int dec_gemv_launch_en(const DecGemvParams &P, int wgs_per_cu_opt, hipStream_t s)
{
    constexpr int NM = epi_is_glu(EPI) ? 2 : 1;
    DecGemvFacts F;
    F.dtype = DT; F.epi = EPI; F.norm = NORM; F.x_add = XADD; F.cols = P.cols; F.total_rows = P.total_rows; F.num_cus = dec_num_cus(); F.rpw = wgs_per_cu_opt;
    const DecGemvPlan R = plan_dec_gemv<DT>(F);
    switch (R.error) {
    case DEC_GEMV_OK: break;
    case DEC_GEMV_ERR_COLS:
        if (P.cols <= 0) return ifa_fail(IFA_ERR_ARG, "fused GEMV: no columns");
        return ifa_fail(IFA_ERR_ARG, "fused GEMV: %d columns are not whole blocks of dtype %d", P.cols, DT);
    case DEC_GEMV_ERR_NO_KERNEL: return ifa_fail(IFA_ERR_ARG, "fused GEMV: no kernel for epilogue %d / norm %d", EPI, NORM);
    case DEC_GEMV_ERR_LONG_LIMIT: return ifa_fail(IFA_ERR_ARG, "fused GEMV: %d columns exceed the limit of dtype %d", P.cols, DT);
    case DEC_GEMV_ERR_PACKED: return ifa_fail(IFA_ERR_ARG, "fused GEMV: grid %d / %d blocks per row exceed the packed launch scalars", R.grid, P.nblk);
    default: return ifa_fail(IFA_ERR_ARG, "fused GEMV: %d columns exceed the limit of dtype %d for a normalised / gated input", P.cols, DT);
    }
    const size_t smem = (size_t)R.lds;
    if (R.kind == DEC_GEMV_LONG) {
        // long rows (w2 / wo of 34B-70B models): chunked kernel, no norm prologue, no GLU pair
        if constexpr (NORM == 0 && !XADD && (EPI == EPI_PLAIN || EPI == EPI_RESIDUAL || EPI == EPI_MOE_ACC || EPI == EPI_MOE_LAST)) {
            constexpr int MJ = DecGemvLimits<DT>::MAXNJ;
#define IFA_DGL(NJV) \
    case NJV: if constexpr (NJV <= MJ) { \
        auto kern = k_dec_gemv_long<DT, NJV, dec_rw_long<DT>(NJV), EPI>; \
        if (smem > 48 * 1024) IFA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
        kern<<<dim3((unsigned)R.grid), dim3(DEC_THREADS), smem, s>>>(P); } break;
            switch (R.njl) { IFA_DGL(1) IFA_DGL(2) IFA_DGL(3) IFA_DGL(4) IFA_DGL(5) IFA_DGL(6) IFA_DGL(7) IFA_DGL(8) }
#undef IFA_DGL
            IFA_LAUNCH_CHECK();
            return IFA_OK;
        } else {
            return ifa_fail(IFA_ERR_ARG, "fused GEMV: %d columns exceed the limit of dtype %d for a normalised / gated input", P.cols, DT);
        }
    }
    // exactly one workgroup per CU (a second one would queue its activation behind the first one's weights)
    const int wgs = R.grid;
    const dim3 grid((unsigned)wgs);
    // the matrix pointer as a preloaded kernel argument when the launch has ONE matrix (pair) and no expert table (k_dec_gemv)
    const uint8_t *pw0 = (P.nsets == 1 && !epi_is_moe(EPI) && !P.w_table) ? P.W0[0] : nullptr;
#ifdef IFA_NO_PRELOAD_W            // (A / B: the row addresses from the argument block, as before round 5)
    pw0 = nullptr;
#endif
    // inputs that are normalised or feed an activation are [dim] vectors (dim <= 8192): <= 4 blocks per lane of a B32 format (the plan refuses more)
    constexpr int NJCAP = (NORM == 1 || EPI == EPI_GLU || EPI == EPI_ACT || EPI == EPI_MOE_GLU || EPI == EPI_MOE_ACT) ? 4 : 8;
#define IFA_DG(NJV) \
    case NJV: if constexpr (NJV <= DecGemvLimits<DT>::MAXNJ && NJV <= NJCAP) { \
        constexpr int THV = dec_threads<DT>(EPI, NORM, NJV, XADD); \
        constexpr int NPV = dec_np<DT>(EPI, NORM, NJV, XADD, THV); \
        auto kern = k_dec_gemv<DT, NJV, dec_rw<DT>(EPI, NORM, NJV, NM, THV), EPI, NORM, XADD, THV, NPV>; \
        if (smem > 48 * 1024) IFA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
        kern<<<grid, dim3(THV), smem, s>>>(P.x, P.norm_w, P.norm_b, P.cols, pw0, P.W1, (int)((unsigned)P.nblk | ((unsigned)wgs << 16)), P.total_rows, P); } break;
    switch (R.nj) { IFA_DG(1) IFA_DG(2) IFA_DG(3) IFA_DG(4) IFA_DG(5) IFA_DG(6) IFA_DG(7) IFA_DG(8) }
#undef IFA_DG
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// the plan of this format's launches, instantiated next to them and nowhere else (plan_dec_gemv and the tables it reads have internal
// linkage; the dispatcher's unit declares the other formats' instances extern): a unit compiled with IFA_T_* overrides plans what it launches
template <int DT>
DecGemvPlan dec_gemv_plan_dt(const DecGemvFacts &f) { return plan_dec_gemv<DT>(f); }

template <int DT>
int dec_gemv_launch_dt(int epi, int norm, const DecGemvParams &P, int wgs_per_cu, hipStream_t s)
{
    if (P.x_add) {      // tensor-parallel seams: the sum of the layer input and the merged product is formed in the prologue
        if (epi == EPI_PLAIN && norm == 1) return dec_gemv_launch_en<DT, EPI_PLAIN, 1, true>(P, wgs_per_cu, s);
        if (epi == EPI_GLU && norm == 1) return dec_gemv_launch_en<DT, EPI_GLU, 1, true>(P, wgs_per_cu, s);
        if (epi == EPI_ACT && norm == 1) return dec_gemv_launch_en<DT, EPI_ACT, 1, true>(P, wgs_per_cu, s);
        return ifa_fail(IFA_ERR_ARG, "fused GEMV: no x_add kernel for epilogue %d / norm %d", epi, norm);
    }
    if (epi == EPI_PLAIN && norm == 1) return dec_gemv_launch_en<DT, EPI_PLAIN, 1>(P, wgs_per_cu, s);
    if (epi == EPI_PLAIN && norm == 0) return dec_gemv_launch_en<DT, EPI_PLAIN, 0>(P, wgs_per_cu, s);
    if (epi == EPI_RESIDUAL && norm == 0) return dec_gemv_launch_en<DT, EPI_RESIDUAL, 0>(P, wgs_per_cu, s);
    if (epi == EPI_RESIDUAL && norm == 2) return dec_gemv_launch_en<DT, EPI_RESIDUAL, 2>(P, wgs_per_cu, s);
    if (epi == EPI_PLAIN && norm == 2) return dec_gemv_launch_en<DT, EPI_PLAIN, 2>(P, wgs_per_cu, s);
    if (epi == EPI_GLU && norm == 1) return dec_gemv_launch_en<DT, EPI_GLU, 1>(P, wgs_per_cu, s);
    if (epi == EPI_ACT && norm == 1) return dec_gemv_launch_en<DT, EPI_ACT, 1>(P, wgs_per_cu, s);
    if (epi == EPI_GLU && norm == 0) return dec_gemv_launch_en<DT, EPI_GLU, 0>(P, wgs_per_cu, s);
    if (epi == EPI_ACT && norm == 0) return dec_gemv_launch_en<DT, EPI_ACT, 0>(P, wgs_per_cu, s);
    if (epi == EPI_MOE_GLU && norm == 1) return dec_gemv_launch_en<DT, EPI_MOE_GLU, 1>(P, wgs_per_cu, s);
    if (epi == EPI_MOE_ACT && norm == 1) return dec_gemv_launch_en<DT, EPI_MOE_ACT, 1>(P, wgs_per_cu, s);
    if (epi == EPI_MOE_ACC && norm == 0) return dec_gemv_launch_en<DT, EPI_MOE_ACC, 0>(P, wgs_per_cu, s);
    if (epi == EPI_MOE_LAST && norm == 0) return dec_gemv_launch_en<DT, EPI_MOE_LAST, 0>(P, wgs_per_cu, s);
    return ifa_fail(IFA_ERR_ARG, "fused GEMV: no kernel for epilogue %d / norm %d", epi, norm);
}

} // namespace ifa
