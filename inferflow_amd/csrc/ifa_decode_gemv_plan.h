// ifa_decode_gemv_plan.h -- which fused decode GEMV instance a launch runs (k_dec_gemv, k_dec_gemv_long, k_dec_gemv_h), with which
// template arguments, grid and LDS size, as pure host functions: no HIP calls, nothing of ifa_model.  The launchers
// (ifa_decode_gemv_impl.h, ifa_dgemv_f16x.hip) take their run-time values from the plan and their template arguments from the same
// dec_rw / dec_threads / dec_np the plan calls; the C ABI exposes it for tests (ifa_decode_gemv_plan, ifa_model_gemv_plan).
#pragma once
#include <algorithm>
#include <cstddef>
#include "ifa_dtype.h"

namespace ifa {

constexpr int DEC_THREADS = 512;   // 8 waves per workgroup
constexpr int DEC_WAVES = DEC_THREADS / 64;
constexpr int DEC_H_ROWS = 2;      // k_dec_gemv_h: rows (EPI_GLU: row pairs) per wave and pass

// EPI_MOE_ACC / EPI_MOE_LAST: y = hfma(product, w_expert, y) (AddByRowIdx_Kernel); LAST also adds the residual(s)
// EPI_MOE_GLU / EPI_MOE_ACT: EPI_GLU / EPI_ACT of an expert.  Only the MOE epilogues contain the table lookup: a
// run-time `if (P.w_table)` in the dense kernels cost them ~2 us each (weight pointers forced through VGPRs).
enum DecEpilogue { EPI_PLAIN = 0, EPI_RESIDUAL = 1, EPI_GLU = 2, EPI_ACT = 3, EPI_MOE_ACC = 4, EPI_MOE_LAST = 5, EPI_MOE_GLU = 6, EPI_MOE_ACT = 7 };
constexpr bool epi_is_moe(int epi) { return epi >= EPI_MOE_ACC; }
constexpr bool epi_is_glu(int epi) { return epi == EPI_GLU || epi == EPI_MOE_GLU; }

// dynamic LDS bytes of the quantised activation image (XLds, ifa_decode_kernels.h): codes [cols], scale and code sum [cols / 32]
// each, 132 partial sums / counters, the staged F16 input [cols]
constexpr size_t xlds_bytes(int cols)
{
    size_t nb = (size_t)cols / 32;
    size_t off = ((size_t)cols + 15) / 16 * 16 + nb * 8;
    off = (off + 15) / 16 * 16;
    off += 132 * 4;
    off = (off + 15) / 16 * 16;
    off += (size_t)cols * 2;
    return off + 16;
}
// k_dec_gemv_h: the F16 activation [cols] and 132 partial sums
constexpr size_t dec_gemv_h_lds_bytes(int cols) { return (((size_t)cols * 2 + 15) & ~(size_t)15) + 132 * 4; }

// blocks-per-lane limit of each format's instantiations (cols <= 64 * capacity * MAXNJ)
template <int DT> struct DecGemvLimits { static constexpr int MAXNJ = 4; };
template <> struct DecGemvLimits<Q4_B32T1A> { static constexpr int MAXNJ = 8; };
template <> struct DecGemvLimits<Q8_B32T2> { static constexpr int MAXNJ = 6; };

// VGPRs one block of one row costs a lane (sizes the rows in flight; DecFmt<DT, NJ>::DW, ifa_decode_kernels.h)
constexpr int dec_fmt_dw(int dt)
{
    return dt == Q4_B32T1A ? 5 : dt == Q3H_NATIVE ? 8 : dt == Q5_B64T1 ? 11 : dt == Q6_B64T1 ? 13 : 9;      // (Q8_B32T2, Q4_B64T1, Q3H_B64T1: 9)
}

// Tuning overrides (tools/sweep_variants.py builds one library per setting): 0 = the table below
#ifndef IFA_T_TH_QKV
#define IFA_T_TH_QKV 0
#endif
#ifndef IFA_T_TH_WO
#define IFA_T_TH_WO 0
#endif
#ifndef IFA_T_TH_GLU
#define IFA_T_TH_GLU 0
#endif
#ifndef IFA_T_TH_W2
#define IFA_T_TH_W2 0
#endif
#ifndef IFA_T_RW_QKV
#define IFA_T_RW_QKV 0
#endif
#ifndef IFA_T_RW_WO
#define IFA_T_RW_WO 0
#endif
#ifndef IFA_T_RW_GLU
#define IFA_T_RW_GLU 0
#endif
#ifndef IFA_T_RW_W2
#define IFA_T_RW_W2 0
#endif

#ifndef IFA_T_NP_QKV
#define IFA_T_NP_QKV -1
#endif
#ifndef IFA_T_NP_GLU
#define IFA_T_NP_GLU -1
#endif
#ifndef IFA_T_NP_W2
#define IFA_T_NP_W2 -1
#endif

// which of the four per-layer kernels a template instance is (by epilogue / prologue), for the overrides above
constexpr int dec_role(int epi, int norm) { return epi == EPI_GLU ? 2 : (epi == EPI_RESIDUAL ? (norm == 2 ? 1 : 3) : (epi == EPI_PLAIN && norm == 1 ? 0 : -1)); }

// (dec_rw / dec_threads / dec_np: static -- see plan_dec_gemv)
// rows (EPI_GLU: row pairs) a wave keeps in flight: bounded by registers, NM * RW * NJ * DW VGPRs
template <int DT>
static constexpr int dec_rw(int epi, int norm, int nj, int nm, int th = DEC_THREADS)
{
    if (DT == Q4_B32T1A) {      // tuned on Llama-2-7B shapes (DESIGN.md "Kernel timeline")
        const int role = dec_role(epi, norm);
        const int forced = role == 0 ? IFA_T_RW_QKV : role == 1 ? IFA_T_RW_WO : role == 2 ? IFA_T_RW_GLU : role == 3 ? IFA_T_RW_W2 : 0;
        if (forced > 0) return forced;
        if (norm == 2 && nj == 2 && nm == 1) return th > DEC_THREADS ? 1 : 2;    // Wo without a prologue: 16 rows per CU, all requested at once (sweep r02)
        constexpr int a[9] = {0, 6, 6, 4, 4, 2, 2, 2, 2}, b[9] = {0, 6, 6, 3, 2, 2, 1, 1, 1};
        const int rw = nm == 2 ? b[nj] : a[nj];
        return th > DEC_THREADS ? (rw + 1) / 2 : rw;       // 1024 threads: 128 registers per lane, half the rows per wave
    }
    {   // (the sweep overrides apply to whichever format's translation unit is compiled with them)
        const int role = dec_role(epi, norm);
        const int forced = role == 0 ? IFA_T_RW_QKV : role == 1 ? IFA_T_RW_WO : role == 2 ? IFA_T_RW_GLU : role == 3 ? IFA_T_RW_W2 : 0;
        if (forced > 0) return forced;
    }
    // B64 formats (one block per lane at 4096 columns): sweep on Llama-2-7B Q3H + Q8 KV (configs[2];
    // profiles/r02_sweep_q3h.log): 544 -> 601 tok/s; the same entries measured on Q4_B64T1 / Q5_B64T1 (Q6_B64T1: 1024 threads spill)
    if (DT == Q3H_B64T1 || DT == Q3H_NATIVE || DT == Q4_B64T1 || DT == Q5_B64T1 || DT == Q6_B64T1) {
        if (DT != Q6_B64T1 && epi == EPI_GLU && nj == 1 && th > DEC_THREADS) return 3;   // W1/W3 at 1024 threads: 16.7 -> 14.1 us (Q3H)
        if ((epi == EPI_RESIDUAL || epi == EPI_PLAIN) && norm == 2 && nj == 1) return 2; // Wo without a prologue: 6.3 -> 4.6 us
        if (epi == EPI_RESIDUAL && norm == 0 && nj == 3) return 2;                    // W2 (11008 columns): 10.4 -> 9.1 us
    }
    if (DT == Q8_B32T2) {       // two blocks per lane at 4096 columns, like Q4_B32T1
        if (epi == EPI_GLU && nj == 2 && th > DEC_THREADS) return 2;
        if ((epi == EPI_RESIDUAL || epi == EPI_PLAIN) && norm == 2 && nj == 2) return 2;
    }
    int rw = 72 / (nm * nj * dec_fmt_dw(DT));
    rw = rw < 1 ? 1 : (rw > 6 ? 6 : rw);
    return th > DEC_THREADS ? (rw + 1) / 2 : rw;           // 1024 threads: 128 registers per lane
}

// k_dec_gemv_long keeps two register sets (software pipeline over the chunks): half the rows of the single-chunk kernel
template <int DT>
static constexpr int dec_rw_long(int njl) { return dec_rw<DT>(-1, 0, njl, 1) >= 2 ? dec_rw<DT>(-1, 0, njl, 1) / 2 : 1; }

// Workgroup size by kernel shape, measured on Llama-2-7B Q4: the gated W1/W3 kernel and the short Wo kernel
// (2 blocks per lane) gain from four waves per SIMD (issue stalls overlap), QKV and the long-row W2 kernel lose
template <int DT>
static constexpr int dec_threads(int epi, int norm, int nj, bool xadd)
{
    if (!xadd) {
        const int role = dec_role(epi, norm);
        const int forced = role == 0 ? IFA_T_TH_QKV : role == 1 ? IFA_T_TH_WO : role == 2 ? IFA_T_TH_GLU : role == 3 ? IFA_T_TH_W2 : 0;
        if (forced > 0) return forced;
    }
    if ((DT == Q3H_B64T1 || DT == Q3H_NATIVE || DT == Q4_B64T1 || DT == Q5_B64T1) && nj == 1 && !xadd && epi == EPI_GLU) return 1024;          // (see dec_rw)
    if (DT == Q8_B32T2 && nj == 2 && !xadd && epi == EPI_GLU) return 1024;
    if (DT == Q4_B32T1A && nj == 2 && !xadd && epi == EPI_PLAIN && norm == 1) return 1024;      // QKV with the wave-specialised prologue (r04 sweep: 8.8 -> 8.3 us)
    return (DT == Q4_B32T1A && nj == 2 && !xadd && (epi == EPI_GLU || (epi == EPI_RESIDUAL && norm == 0))) ? 1024 : DEC_THREADS;
}

// waves that run the norm / quantiser prologue while the others already stream their rows (k_dec_gemv's NP; 0 = every wave
// takes part in the prologue, the round 1-3 form).  Only the dense per-layer kernels with a prologue.
template <int DT>
static constexpr int dec_np(int epi, int norm, int nj, bool xadd, int th)
{
    if (xadd || norm == 2) return 0;
    const int role = dec_role(epi, norm);
    const int forced = role == 0 ? IFA_T_NP_QKV : role == 2 ? IFA_T_NP_GLU : role == 3 ? IFA_T_NP_W2 : -1;
    if (forced >= 0) return forced < th / 64 ? forced : 0;
    // round-4 sweep on Llama-2-7B Q4 (DESIGN.md section 3 "wave-specialised prologue"): half of the waves
    // run the prologue -- QKV 9.6 -> 8.2-8.5 us (1024 threads), W1/W3 13.1 -> 12.95, W2 9.05 -> 8.0-8.1 (512 threads);
    // a quarter or three quarters of the waves lose (the prologue's VALU time, or too few early requests)
    if (role == 0 || role == 2 || role == 3) return th / 128;
    return 0;
}

// ------------------------------------------------------------------ the plan
// What the decision reads.  The order of the fields is the order of ifa_decode_gemv_plan's `facts` array.
struct DecGemvFacts {
    int dtype = 0;                       // the weight format (Q4_B32T1B runs Q4_B32T1A's instances; Q3H_NATIVE: option q3h_native)
    int epi = 0, norm = 0, x_add = 0;    // DecEpilogue; 0 no norm, 1 RMS-norm prologue, 2 the activation arrives quantised; tensor-parallel seam
    int cols = 0, total_rows = 0;        // total_rows: rows of all sets (EPI_GLU: row pairs)
    int num_cus = 0;
    int rpw = 0;                         // the rpw_* option: workgroups per CU, 0 = one
};
enum DecGemvKind { DEC_GEMV_NONE = 0, DEC_GEMV_CLASSIC = 1, DEC_GEMV_LONG = 2, DEC_GEMV_F16X = 3 };
enum DecGemvPlanError {
    DEC_GEMV_OK = 0,
    DEC_GEMV_ERR_DTYPE = 1,              // no fused kernel for this weight format
    DEC_GEMV_ERR_COLS = 2,               // no columns, or not whole blocks (fp16 activations: not whole 8-value chunks)
    DEC_GEMV_ERR_LONG_LIMIT = 3,         // more than 4 chunks of MAXNJ blocks per lane, or more than 32768 columns
    DEC_GEMV_ERR_NJ_INPUT = 4,           // more blocks per lane than a normalised / gated input may have (4), or than MAXNJ where no long kernel exists
    DEC_GEMV_ERR_PACKED = 5,             // grid or blocks per row exceed the 16-bit halves of the packed launch scalar
    DEC_GEMV_ERR_NO_KERNEL = 6,          // no instance for this epilogue / norm / x_add combination
};

// What a launch runs.  The order of the fields is the order of ifa_decode_gemv_plan's `out` array.
struct DecGemvPlan {
    int kind = DEC_GEMV_NONE;
    int nj = 0;                          // blocks per lane of a whole row, ceil(cols / (64 * capacity)) (fp16 activations: lane-loop rounds -- 256 chunks of 8 for F16, 64 blocks else)
    int nchunk = 0, njl = 0;             // Long: register chunks per row, blocks per lane and chunk (the NJ of the instance)
    int rw = 0, threads = 0, np = 0;     // the RW / TH / NP template arguments of the instance
    int grid = 0, waves = 0, npass = 0;  // workgroups; W = grid * threads / 64; passes of rw * W rows
    int partial = 0;                     // the last pass has fewer than rw * W rows
    int lds = 0;                         // dynamic LDS bytes
    int error = DEC_GEMV_OK;
};
constexpr int DEC_GEMV_N_FACTS = sizeof(DecGemvFacts) / sizeof(int), DEC_GEMV_N_OUT = sizeof(DecGemvPlan) / sizeof(int);      // 8, 13

// the (epilogue, norm, x_add) combinations dec_gemv_launch_dt instantiates
constexpr bool dec_gemv_has_kernel(int epi, int norm, bool xadd)
{
    if (xadd) return norm == 1 && (epi == EPI_PLAIN || epi == EPI_GLU || epi == EPI_ACT);
    if (norm == 2) return epi == EPI_PLAIN || epi == EPI_RESIDUAL;
    if (norm == 1) return epi == EPI_PLAIN || epi == EPI_GLU || epi == EPI_ACT || epi == EPI_MOE_GLU || epi == EPI_MOE_ACT;
    return norm == 0 && (epi == EPI_PLAIN || epi == EPI_RESIDUAL || epi == EPI_GLU || epi == EPI_ACT || epi == EPI_MOE_ACC || epi == EPI_MOE_LAST);
}
// the same for launch_h_dt (ifa_dgemv_f16x.hip)
constexpr bool dec_gemv_h_has_kernel(int epi, int norm, bool xadd)
{
    if (xadd) return norm == 1 && (epi == EPI_PLAIN || epi == EPI_GLU || epi == EPI_ACT);
    if (norm == 1) return epi == EPI_PLAIN || epi == EPI_GLU || epi == EPI_ACT;
    return norm == 0 && (epi == EPI_PLAIN || epi == EPI_RESIDUAL || epi == EPI_GLU || epi == EPI_ACT);
}

inline void dec_gemv_plan_passes(DecGemvPlan &r, int total_rows)
{
    r.waves = r.grid * (r.threads / 64);
    const long long per_pass = (long long)r.rw * r.waves;
    r.npass = (int)((total_rows + per_pass - 1) / per_pass);
    r.partial = (long long)r.npass * per_pass != total_rows;
}

// The int8-path kernels of format DT (k_dec_gemv / k_dec_gemv_long).  f.dtype is not read: the caller chose DT.
// Internal linkage, like the tables above: their values depend on the IFA_T_* overrides a translation unit is compiled with, so no
// two units may share one copy.
template <int DT>
static DecGemvPlan plan_dec_gemv(const DecGemvFacts &f)
{
    constexpr int MJ = DecGemvLimits<DT>::MAXNJ;
    const int cap = block_capacity(DT);
    const bool xadd = f.x_add != 0;
    DecGemvPlan r;
    auto refuse = [&](int e) { r.kind = DEC_GEMV_NONE; r.error = e; return r; };
    if (f.cols <= 0 || f.cols % cap != 0) return refuse(DEC_GEMV_ERR_COLS);
    const int nblk = f.cols / cap;
    r.nj = (nblk + 63) / 64;
    if (f.cols > 32768 || r.nj > 4 * MJ) return refuse(DEC_GEMV_ERR_LONG_LIMIT);
    if (!dec_gemv_has_kernel(f.epi, f.norm, xadd)) return refuse(DEC_GEMV_ERR_NO_KERNEL);
    const int per_cu = f.rpw > 0 ? f.rpw : 1;
    const int nm = epi_is_glu(f.epi) ? 2 : 1;
    r.lds = (int)xlds_bytes(f.cols);
    if (r.nj > MJ) {
        // long rows (w2 / wo of 34B-70B models): chunked kernel, no norm prologue, no GLU pair
        const bool long_ok = f.norm == 0 && !xadd && (f.epi == EPI_PLAIN || f.epi == EPI_RESIDUAL || f.epi == EPI_MOE_ACC || f.epi == EPI_MOE_LAST);
        if (!long_ok) return refuse(DEC_GEMV_ERR_NJ_INPUT);
        r.kind = DEC_GEMV_LONG;
        r.nchunk = (r.nj + MJ - 1) / MJ;
        r.njl = (r.nj + r.nchunk - 1) / r.nchunk;
        r.threads = DEC_THREADS; r.np = 0;
        r.rw = dec_rw_long<DT>(r.njl);
        r.grid = std::max(1, std::min(f.num_cus * per_cu, (f.total_rows + DEC_WAVES - 1) / DEC_WAVES));
        dec_gemv_plan_passes(r, f.total_rows);
        return r;
    }
    // exactly one workgroup per CU (a second one would queue its activation behind the first one's weights)
    r.kind = DEC_GEMV_CLASSIC;
    r.nchunk = 1; r.njl = r.nj;
    r.threads = dec_threads<DT>(f.epi, f.norm, r.nj, xadd);
    r.np = dec_np<DT>(f.epi, f.norm, r.nj, xadd, r.threads);
    r.rw = dec_rw<DT>(f.epi, f.norm, r.nj, nm, r.threads);
    const int waves = r.threads / 64;
    r.grid = std::max(1, std::min(f.num_cus * per_cu, (f.total_rows + waves - 1) / waves));
    if (r.grid > 0xFFFF || nblk > 0xFFFF) return refuse(DEC_GEMV_ERR_PACKED);
    // inputs that are normalised or feed an activation are [dim] vectors (dim <= 8192): <= 4 blocks per lane of a B32 format
    const int njcap = (f.norm == 1 || f.epi == EPI_GLU || f.epi == EPI_ACT || f.epi == EPI_MOE_GLU || f.epi == EPI_MOE_ACT) ? 4 : 8;
    if (r.nj > njcap) return refuse(DEC_GEMV_ERR_NJ_INPUT);
    dec_gemv_plan_passes(r, f.total_rows);
    return r;
}

// true if k_dec_gemv_h can stream a [rows][cols] tensor of this dtype: whole blocks, whole 8-value chunks, <= 32768 columns
constexpr bool dec_gemv_h_cols_ok(int w_dtype, size_t cols)
{
    return !(w_dtype == F32 || cols == 0 || cols > 32768 || cols % 8 != 0) && block_capacity(w_dtype) > 0 && cols % (size_t)block_capacity(w_dtype) == 0;
}

// The fp16-activation kernel (k_dec_gemv_h): F16 tensors and the block formats outside the int8 path
inline DecGemvPlan plan_dec_gemv_h(const DecGemvFacts &f)
{
    DecGemvPlan r;
    auto refuse = [&](int e) { r.kind = DEC_GEMV_NONE; r.error = e; return r; };
    if (f.dtype == F32 || block_capacity(f.dtype) <= 0 || f.dtype == Q3H_NATIVE) return refuse(DEC_GEMV_ERR_DTYPE);
    if (f.cols > 32768) return refuse(DEC_GEMV_ERR_LONG_LIMIT);
    if (f.cols <= 0 || !dec_gemv_h_cols_ok(f.dtype, (size_t)f.cols)) return refuse(DEC_GEMV_ERR_COLS);
    if (!dec_gemv_h_has_kernel(f.epi, f.norm, f.x_add != 0)) return refuse(DEC_GEMV_ERR_NO_KERNEL);
    r.kind = DEC_GEMV_F16X;
    r.nj = f.dtype == F16 ? (f.cols / 8 + 255) / 256 : (f.cols / block_capacity(f.dtype) + 63) / 64;
    r.rw = DEC_H_ROWS; r.threads = DEC_THREADS; r.np = 0;
    const int per_wg = DEC_WAVES * DEC_H_ROWS;
    r.grid = std::max(1, std::min(f.num_cus * 2, (f.total_rows + per_wg - 1) / per_wg));
    r.lds = (int)dec_gemv_h_lds_bytes(f.cols);
    dec_gemv_plan_passes(r, f.total_rows);
    return r;
}

// (by the run-time dtype: dec_gemv_plan, ifa_decode_gemv.h -- each format's plan is instantiated in the translation unit that
//  instantiates its kernels, so a unit compiled with IFA_T_* overrides plans what it launches)

} // namespace ifa
