// ifa_gemm_rows_i8.hip -- Y[T][N] = X[T][K] . W[N][K]^T for 2..32 rows over tiled Q4_B32T1 weights, in the arithmetic of the
// single-token step (the reference's T = 1 branch) instead of the dequantise + F16 product of k_gemm_rows_mfma: every token row is
// quantised to Q8_B32T2, every 32-weight block's integer dot product comes out of ONE v_mfma_i32_16x16x32_i8 with a zero accumulator,
// and the fp32 terms xs * (dot * scale + xsum * base) are added in the order of the decode GEMV (ifa_gemv.hip, k_gemv_q4b32 /
// WRowQ4::dot): blocks b = c (mod 64) ascending into class c -- the GEMV's lane c --, the 64 classes in the tree of wave_sum, then
// finish_row and the decode epilogues.  Row t of a launch is therefore bit for bit ifa_gemv_tiled of ifa_quantize_act_q8 of row t,
// whatever T is and wherever the row stands.  docs/rows_gemm_int8.md has the layout and the numbers.
//
// Split of the work.  grid = (token tiles of up to 16 rows -- as many as the LDS holds at this K, the plan decides --, groups of 1..8 consecutive 16-row weight tiles); 8 waves.
//   * prologue: the workgroup's <= 16 token rows are (normalised and) quantised into LDS -- per row K int8 codes, then xs and xsum
//     per block (fp32).  The codes of every 8 elements are stored evens first (e0 e2 e4 e6 e1 e3 e5 e7): that is the order in which
//     `word & 0x0F0F0F0F | (word >> 4 & 0x0F0F0F0F) << 32` leaves the weights' nibbles, so a B operand is one ds_read_b64 and an A
//     operand two ANDs and a shift -- no F16 conversion.  Integer sums are order-free.
//   * wave w owns the classes 8w .. 8w + 7: of every round of 64 blocks it streams eight consecutive blocks of its tile's 16 rows --
//     lane (g = lane / 16, i = lane % 16) the four code bytes 4g .. 4g + 3 of row i (its A operand: k = 8g .. 8g + 7 of the block) and,
//     as two 16-byte reads per row, the (base, scale) words of rows 4g .. 4g + 3: the rows whose sums the MFMA leaves in this lane.
//   * the three first levels of the wave_sum tree join classes of one wave (registers), the three last ones join waves (LDS); thread
//     (token, row) of the workgroup then finishes one output.
//   * the next round's codes and words are requested before the current round's MFMAs.
// No waits between workgroups, no K parts: every workgroup walks all of K for its tiles.
#include <algorithm>
#include <cstring>
#include "ifa_host.h"
#include "ifa_decode_kernels.h"
#include "ifa_gemm_rows_i8.h"

namespace ifa {

typedef int gi_i32x4 __attribute__((ext_vector_type(4)));

// one weight tile of the virtual row space: the set it lies in (sets are whole tiles when there are several)
struct GiTile { int si, row0, rows; const uint8_t *W; };
__device__ __forceinline__ GiTile gi_locate(const GmArgs &P, int tile, int m)
{
    const int v = tile * 16, r0 = P.rows[0], r1 = P.rows[1];
    const bool in1 = P.nsets > 1 && v >= r0, in2 = P.nsets > 2 && v >= r0 + r1;
    GiTile t;
    t.si = in2 ? 2 : (in1 ? 1 : 0);
    t.row0 = in2 ? v - r0 - r1 : (in1 ? v - r0 : v);
    t.rows = in2 ? P.rows[2] : (in1 ? r1 : r0);
    t.W = m ? P.Wt1 : (in2 ? P.Wt[2] : (in1 ? P.Wt[1] : P.Wt[0]));
    return t;
}

template <int EPI, int NORM>
__global__ void __launch_bounds__(GI_THREADS) k_gemm_rows_i8(const GmArgs P, int tiles_per_wg, int ntiles, int row_stride, int tokens_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NM = EPI == GM_GLU ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk = P.nblk, K = nblk * 32, chunks = K >> 3;
    const int t0 = blockIdx.x * tokens_per_wg, nt = min(tokens_per_wg, P.T - t0);      // this workgroup's token rows (<= 16)
    const int tile0 = blockIdx.y * tiles_per_wg, ntl = min(tiles_per_wg, ntiles - tile0);
    float *parts = reinterpret_cast<float *>(smem + (size_t)nt * row_stride);     // [NM][wave][4][64]
    float *nsum = parts + NM * GI_WAVES * 256;                                     // [token][wave]
    const size_t row_bytes = tiled_row_bytes(Q4_B32T1A, (size_t)nblk);
    const int nr = (nblk + 63) >> 6, nsteps = ntl * NM * nr;

    // ---- the weight stream: one step = one round of 64 blocks of one matrix of one tile.  Every address is clamped into its matrix
    // (rows past a ragged last tile, blocks past the row end): what a clamped request returns is never used
    struct Slice { uint32_t c[8]; u32x4 sb[4][2]; };
    auto fetch = [&](Slice &sl, int step) {
        const int ti = step / (NM * nr), rem = step - ti * (NM * nr), m = rem / nr, rho = rem - m * nr;
        const GiTile t = gi_locate(P, tile0 + ti, m);
        const int b0 = rho * 64 + wave * 8;
        const uint8_t *wr = t.W + (size_t)min(t.row0 + (lane & 15), t.rows - 1) * row_bytes + 4 * g;
#pragma unroll
        for (int i = 0; i < 8; i++) sl.c[i] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(wr + (size_t)min(b0 + i, nblk - 1) * 16));
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint8_t *wq = t.W + (size_t)min(t.row0 + 4 * g + r, t.rows - 1) * row_bytes + (size_t)nblk * 16;
#pragma unroll
            for (int h = 0; h < 2; h++) sl.sb[r][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wq + (size_t)min(b0 + 4 * h, nblk - 4) * 4));
        }
    };
    Slice cur, nxt;
    fetch(cur, 0);

    // ---- prologue: token rows -> Q8_B32T2 in LDS.  The quantiser is XPre::finish's (ifa_decode_kernels.h), a block = the four lanes
    // of a quad; the norm's statistics in the order of ifa_math.h: chunk c = tid is lane c % 64 of group c / 64 = wave (K <= 4096)
    if constexpr (NORM == 1) {
        for (int t = 0; t < nt; t++) {
            half8_t v;
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = (half_t)0;
            if (tid < chunks) v = *reinterpret_cast<const half8_t *>(P.X + (size_t)(t0 + t) * P.ldx + (size_t)tid * 8);
            const float pg = wave_sum(rms_chunk_sq(v));
            if (lane == 0) nsum[t * GI_WAVES + wave] = pg;
        }
        __syncthreads();
    }
    for (int t = 0; t < nt; t++) {
        char *img = smem + (size_t)t * row_stride;
        float *xs_img = reinterpret_cast<float *>(img + K), *xsum_img = xs_img + nblk;
        float nscale = 1.0f;
        if constexpr (NORM == 1) {
            const int ng = (chunks + 63) >> 6;
            float total = 0.0f;
#pragma unroll
            for (int w = 0; w < GI_WAVES; w++) total = total + (w < ng ? nsum[t * GI_WAVES + w] : 0.0f);
            nscale = rms_scale_of(total, K, P.eps);
        }
        for (int c = tid; c < chunks; c += GI_THREADS) {      // whole quads (= blocks) are in or out together: K % 32 == 0
            const half8_t xv = *reinterpret_cast<const half8_t *>(P.X + (size_t)(t0 + t) * P.ldx + (size_t)c * 8);
            float v[8];
            if constexpr (NORM == 1) {
                half8_t wv;
                if (P.norm_w) wv = *reinterpret_cast<const half8_t *>(P.norm_w + (size_t)c * 8);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    float a = (float)xv[i] * nscale;
                    if (P.norm_w) { const float mw = P.multi_base + (float)wv[i]; a = a * mw; }
                    v[i] = h2f(f2h(a));
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = (float)xv[i];
            }
            float mx = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; i++) mx = fmaxf(mx, fabsf(v[i]));
            mx = fmaxf(mx, dpp_xor1(mx));
            mx = fmaxf(mx, dpp_xor2(mx));
            const float qs = mx / 127;
            int q[8], s = 0;
            q8_round_div8(v, qs, q);
#pragma unroll
            for (int i = 0; i < 8; i++) s += q[i];
            s += dpp_xor1(s);
            s += dpp_xor2(s);
            u32x2 packed;      // evens, then odds: the order of the weights' nibbles in an A operand
            packed[0] = (uint32_t)(q[0] & 0xFF) | ((uint32_t)(q[2] & 0xFF) << 8) | ((uint32_t)(q[4] & 0xFF) << 16) | ((uint32_t)(q[6] & 0xFF) << 24);
            packed[1] = (uint32_t)(q[1] & 0xFF) | ((uint32_t)(q[3] & 0xFF) << 8) | ((uint32_t)(q[5] & 0xFF) << 16) | ((uint32_t)(q[7] & 0xFF) << 24);
            *reinterpret_cast<u32x2 *>(img + (size_t)c * 8) = packed;
            if ((c & 3) == 0) {
                xs_img[c >> 2] = h2f(f2h(qs));      // the fp16-rounded scale is what the GEMV multiplies by
                xsum_img[c >> 2] = (float)s;
            }
        }
    }
    __syncthreads();

    // ---- the tiles.  Lane (g, i): A = row i of the tile, B = token i (rows past nt: token nt - 1 again, never stored); the MFMA leaves
    // dot[r] = weight row 4g + r x token i in this lane
    const char *img = smem + (size_t)min(lane & 15, nt - 1) * row_stride;
    const float *xs_img = reinterpret_cast<const float *>(img + K), *xsum_img = xs_img + nblk;
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[i][r] = 0.0f;
    for (int step = 0; step < nsteps; step++) {
        if (step + 1 < nsteps) fetch(nxt, step + 1);
        const int ti = step / (NM * nr), rem = step - ti * (NM * nr), m = rem / nr, rho = rem - m * nr;
        const int b0 = rho * 64 + wave * 8;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int blk = b0 + i;
            if (blk >= nblk) break;      // (wave-uniform) a class without a block in this round adds nothing: the GEMV's idle lane
            const uint32_t cw = cur.c[i];
            const uint64_t a = (uint64_t)(cw & 0x0F0F0F0Fu) | ((uint64_t)((cw >> 4) & 0x0F0F0F0Fu) << 32);
            const uint64_t b = *reinterpret_cast<const uint64_t *>(img + (size_t)blk * 32 + 8 * g);
            const float xs = xs_img[blk], xsum = xsum_img[blk];
            const gi_i32x4 d = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)a, (long)b, gi_i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t word = cur.sb[r][i >> 2][i & 3];
                const float base = hbits2f((uint16_t)(word & 0xFFFFu)), scale = hbits2f((uint16_t)(word >> 16));
                // k_gemv_q4b32's expression; the library is built without contraction, so its multiplies and adds are separate roundings
                const float tt = __fadd_rn(__fmul_rn((float)d[r], scale), __fmul_rn(xsum, base));
                acc[i][r] = __fadd_rn(acc[i][r], __fmul_rn(xs, tt));
            }
        }
        cur = nxt;
        if (rho + 1 < nr) continue;
        // ---- the matrix is through for this tile: wave_sum's levels xor 1, xor 2, half mirror over this wave's eight classes
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float s = __fadd_rn(__fadd_rn(__fadd_rn(acc[0][r], acc[1][r]), __fadd_rn(acc[2][r], acc[3][r])),
                                      __fadd_rn(__fadd_rn(acc[4][r], acc[5][r]), __fadd_rn(acc[6][r], acc[7][r])));
            parts[((m * GI_WAVES + wave) * 4 + r) * 64 + lane] = s;
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i][r] = 0.0f;
        }
        if (m + 1 < NM) continue;
        __syncthreads();
        // ---- thread (token = tid / 16, row = tid % 16) finishes one output: the levels row mirror, xor 16, xor 32 join the waves
        const GiTile t = gi_locate(P, tile0 + ti, 0);
        const int row = t.row0 + (tid & 15), tok = tid >> 4;
        if (tid < 256 && tok < nt && row < t.rows) {
            const int src = ((tid & 15) & 3) * 64 + ((tid & 15) >> 2) * 16 + tok;
            float a[NM];
#pragma unroll
            for (int mm = 0; mm < NM; mm++) {
                const float *p = parts + (size_t)mm * GI_WAVES * 256 + src;
                a[mm] = __fadd_rn(__fadd_rn(__fadd_rn(p[0], p[256]), __fadd_rn(p[512], p[768])),
                                  __fadd_rn(__fadd_rn(p[1024], p[1280]), __fadd_rn(p[1536], p[1792])));
            }
            const half_t *bias = t.si == 2 ? P.bias[2] : (t.si == 1 ? P.bias[1] : P.bias[0]);
            half_t y = dec_bias(a[0], bias, row);
            const int vrow = tile0 * 16 + ti * 16 + (tid & 15), trow = t0 + tok;
            if constexpr (EPI == GM_RESIDUAL) {
                y = f2h(h2f(P.res[(size_t)trow * P.ldres + vrow]) + h2f(y));      // TensorOpr::Add (EPI_RESIDUAL of the decode GEMV)
            } else if constexpr (EPI == GM_GLU) {
                const half_t t2 = dec_bias(a[NM - 1], P.bias1, row);
                const half_t act = f2h(act_fn(h2f(y), P.act_kind));               // TensorOpr::Activation -> F16
                y = f2h(h2f(act) * h2f(t2));                                      // TensorOpr::Mul (EPI_GLU)
            }
            half_t *ys = t.si == 2 ? P.Yset[2] : (t.si == 1 ? P.Yset[1] : P.Yset[0]);
            const int lds = t.si == 2 ? P.ldyset[2] : (t.si == 1 ? P.ldyset[1] : P.ldyset[0]);
            if (ys) ys[(size_t)trow * lds + row] = y;
            else P.Y[(size_t)trow * P.ldy + vrow] = y;
        }
        __syncthreads();      // the partial sums have been read before the next tile's are written
    }
}

static int gi_num_cus()
{
    static int n = 0;
    if (!n) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

GemmRowsI8Facts gemm_rows_i8_facts(int w_dtype, const GmArgs &P, int epi, int norm)
{
    GemmRowsI8Facts f;
    f.T = P.T; f.w_dtype = w_dtype; f.cols = P.nblk * 32; f.nsets = P.nsets; f.rows0 = P.rows[0]; f.rows1 = P.rows[1]; f.rows2 = P.rows[2];
    f.epi = epi; f.norm = norm; f.has_w1 = P.Wt1 != nullptr; f.num_cus = gi_num_cus();
    return f;
}

bool gemm_rows_i8_ok(int w_dtype, const GmArgs &P, int epi, int norm)
{
    return plan_gemm_rows_i8(gemm_rows_i8_facts(w_dtype, P, epi, norm)).error == GEMM_ROWS_I8_OK;
}

template <int EPI, int NORM>
static int gi_launch(const GmArgs &P, const GemmRowsI8Plan &plan, hipStream_t s)
{
    auto kern = k_gemm_rows_i8<EPI, NORM>;
    if (plan.lds > 48 * 1024) IFA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, plan.lds));
    kern<<<dim3((unsigned)plan.token_tiles, (unsigned)plan.grid), dim3(GI_THREADS), (size_t)plan.lds, s>>>(P, plan.tiles_per_wg, plan.ntiles, plan.row_stride, plan.tokens_per_wg);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

int gemm_rows_i8_launch(int w_dtype, const GmArgs &P0, int epi, int norm, hipStream_t s, int num_cus)
{
    GemmRowsI8Facts f = gemm_rows_i8_facts(w_dtype, P0, epi, norm);
    if (num_cus > 0) f.num_cus = num_cus;      // (a caller that plans for fewer CUs: more tiles per workgroup)
    const GemmRowsI8Plan plan = plan_gemm_rows_i8(f);
    if (plan.error) return ifa_fail(IFA_ERR_ARG, "int8 rows GEMM: launch refused (T %d, %d blocks, %d sets, epilogue %d, norm %d; plan error %d)", P0.T, P0.nblk, P0.nsets, epi, norm, plan.error);
    GmArgs P = P0;
    P.total_rows = plan.total_rows;
    if (epi == GM_PLAIN) return norm ? gi_launch<GM_PLAIN, 1>(P, plan, s) : gi_launch<GM_PLAIN, 0>(P, plan, s);
    if (epi == GM_RESIDUAL) return norm ? gi_launch<GM_RESIDUAL, 1>(P, plan, s) : gi_launch<GM_RESIDUAL, 0>(P, plan, s);
    return norm ? gi_launch<GM_GLU, 1>(P, plan, s) : gi_launch<GM_GLU, 0>(P, plan, s);
}

} // namespace ifa

using namespace ifa;

extern "C" {

int ifa_gemm_rows_i8_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == GEMM_ROWS_I8_N_FACTS && n_out >= GEMM_ROWS_I8_N_OUT, "ifa_gemm_rows_i8_plan: %d facts, %d outputs expected", GEMM_ROWS_I8_N_FACTS,
                GEMM_ROWS_I8_N_OUT);
    GemmRowsI8Facts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.num_cus >= 1, "ifa_gemm_rows_i8_plan: num_cus %d", f.num_cus);
    const GemmRowsI8Plan r = plan_gemm_rows_i8(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_gemm_rows_q8(int w_dtype, const void *const Wt_tiled[3], const int rows[3], int nsets, const void *W1_tiled, size_t cols, const void *x_f16, int ldx, int T,
                     int epi, int norm, const void *norm_w_f16, float multi_base, float eps, const void *const bias_f16[3], const void *bias1_f16, const void *res_f16,
                     int ldres, int act_kind, void *y_f16, int ldy, void *const yset_f16[3], int num_cus, ifa_stream stream)
{
    IFA_REQUIRE(Wt_tiled && rows && x_f16 && (y_f16 || yset_f16) && nsets >= 1 && nsets <= 3, "ifa_gemm_rows_q8: null pointer or %d sets", nsets);
    IFA_REQUIRE(cols > 0 && cols < (1u << 24) && ldx >= (int)cols, "ifa_gemm_rows_q8: %zu columns, row stride %d", cols, ldx);
    IFA_REQUIRE(ldx % 8 == 0 && (reinterpret_cast<uintptr_t>(x_f16) & 15) == 0 && (reinterpret_cast<uintptr_t>(norm_w_f16) & 15) == 0 && num_cus >= 0,
                "ifa_gemm_rows_q8: x / norm_w are read 16 bytes at a time (16-byte aligned, row stride %d %% 8 == 0); num_cus %d", ldx, num_cus);
    IFA_REQUIRE(epi != GM_RESIDUAL || (res_f16 && ldres > 0), "ifa_gemm_rows_q8: the residual epilogue needs res");
    GmArgs P;
    memset(&P, 0, sizeof(P));
    int total = 0;
    for (int i = 0; i < nsets; i++) {
        IFA_REQUIRE(Wt_tiled[i] && (!yset_f16 || yset_f16[i]), "ifa_gemm_rows_q8: set %d: null pointer", i);
        P.Wt[i] = (const uint8_t *)Wt_tiled[i]; P.rows[i] = rows[i]; P.bias[i] = bias_f16 ? (const half_t *)bias_f16[i] : nullptr;
        if (yset_f16) { P.Yset[i] = (half_t *)yset_f16[i]; P.ldyset[i] = rows[i]; }
        total += rows[i];
    }
    IFA_REQUIRE(yset_f16 || ldy >= total, "ifa_gemm_rows_q8: %d rows, output stride %d", total, ldy);
    IFA_REQUIRE(epi != GM_RESIDUAL || ldres >= total, "ifa_gemm_rows_q8: %d rows, residual stride %d", total, ldres);
    P.Wt1 = (const uint8_t *)W1_tiled; P.bias1 = (const half_t *)bias1_f16; P.nsets = nsets; P.nblk = (int)(cols / 32); P.T = T;
    P.X = (const half_t *)x_f16; P.ldx = ldx; P.multi_base = multi_base; P.eps = eps; P.norm_w = (const half_t *)norm_w_f16;
    P.Y = (half_t *)y_f16; P.ldy = ldy; P.res = (const half_t *)res_f16; P.ldres = ldres; P.act_kind = act_kind; P.i8 = 1;
    IFA_REQUIRE(cols % 32 == 0, "ifa_gemm_rows_q8: %zu columns are no whole blocks", cols);
    return gemm_rows_i8_launch(w_dtype, P, epi, norm, ifa_s(stream), num_cus);
}

} // extern "C"
