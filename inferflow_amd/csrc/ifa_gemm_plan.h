// ifa_gemm_plan.h -- what a prompt GEMM launch runs: k_gemm_mid (ifa_gemm_mid.hip) -- token tile, parts of K in the order they are
// tried, grid and LDS bytes of each -- and k_gemm_big (ifa_gemm.hip) -- tile shape, one or two launches, waves, split-K candidates --
// as pure host functions: no HIP calls, nothing of GmArgs.  The launchers (md_launch, launch_gemm_big) take their run-time values from
// the plan and their template arguments from the same constants; the C ABI exposes both for tests (ifa_gemm_mid_plan,
// ifa_gemm_big_plan).  The measurements behind every number are in the launchers' comments and in DESIGN.md.
#pragma once
#include <algorithm>
#include <cstddef>
#include "ifa_dtype.h"

namespace ifa {

enum GemmPlanEpilogue { GP_PLAIN = 0, GP_RESIDUAL = 1, GP_GLU = 2 };      // == GmEpilogue (ifa_gemm_rows_mfma.h)

// ------------------------------------------------------------------ k_gemm_mid
#ifndef IFA_MID_NS
#define IFA_MID_NS 3        // stages of the direct-to-LDS ring
#endif
constexpr int MD_BN = 128, MD_BK = 64, MD_NW = 4, MD_NT = 256;      // weight rows of a tile, columns of a step, computing waves, their threads (token rows of a tile: 32 TA)
constexpr int md_a_bytes(int ta) { return 32 * ta * MD_BK * 2; }       // activation tile of a step (TA = 4: 16 KB), rows of 128 bytes, 16-byte chunks swizzled
constexpr int MD_WC_BYTES = MD_NW * 1024, MD_WS_BYTES = MD_NW * 256; // raw codes (32 rows x 2 blocks x 16 B per wave), (base, scale) words
constexpr int md_stage(int ta) { return md_a_bytes(ta) + MD_WC_BYTES + MD_WS_BYTES; }    // 21 KB (TA = 4) / 37 KB (TA = 8)
constexpr size_t md_lds_bytes(int ta) { return std::max((size_t)IFA_MID_NS * md_stage(ta), (size_t)(32 * ta) * (MD_BN * 2 + 64)); }      // the ring; the epilogue's output tile
constexpr int MD_MAX_TRIES = 5;

// What the decision reads.  The order of the fields is the order of ifa_gemm_mid_plan's `facts` array.
struct GemmMidFacts {
    int T = 0;
    int nsets = 1, rows0 = 0, rows1 = 0, rows2 = 0;      // weight rows of each set (the gated pair: rows of w1 = rows of w3)
    int nblk = 0;                        // 32-weight blocks per row (K / 32)
    int epi = GP_PLAIN;
    int num_cus = 0;
    int no_waits = 0;                    // GmArgs::no_waits: the caller's veto of launches that wait
    int waits_on = 1;                    // waits_enabled() (ifa_host.h)
    // the measurement settings (0 = the default; md_settings, ifa_gemm_mid.hip, fills them from the environment once)
    int max_parts = 0;                   // widest part count allowed (default 8; 16 exists for TA = 4 only)
    int ta = 0;                          // 32-token accumulator tiles of a wave: 4 (default) or 8
    int min_steps = 0;                   // least 64-column steps of a part (default 4)
    int two_per_cu = 0;                  // cap of 2 workgroups per CU for every epilogue (the gated pair always has it)
    int no_glu_split = 0;                // the gated pair as one part of K
    // what gemm_mid_ok reads besides
    int mo = 1, has_w1 = 1;              // GmArgs::mo; the gated pair's second matrix is there
    int ld_or = 0;                       // ldx | ldy (or the three ldyset) | ldres where it is read: every stride % 8 == 0
};
enum GemmMidPlanError {
    GEMM_MID_OK = 0,
    GEMM_MID_ERR_LAYOUT = 1,             // the weights are not MO copies
    GEMM_MID_ERR_SHAPE = 2,              // T < 1, not 1..3 sets, fewer than 8 blocks per row or not whole 128-column supersteps
    GEMM_MID_ERR_ROWS = 3,               // a set's rows % 16 != 0
    GEMM_MID_ERR_GLU = 4,                // the gated pair needs one set and W1
    GEMM_MID_ERR_STRIDE = 5,             // a stride % 8 != 0
};
// What a launch runs.  The order of the fields is the order of ifa_gemm_mid_plan's `out` array.
struct GemmMidPlan {
    int error = GEMM_MID_OK;
    int ta = 0;
    int tiles_m = 0, tiles_n = 0;        // token tiles of 32 TA rows; weight tiles of 128 rows (the gated pair: 64 of w1 + 64 of w3) of all sets
    int tile0[4] = {0, 0, 0, 0};         // first weight tile of sets 0 .. 2 (absent sets: 1 << 30: never selected); [3] = tiles_n
    int ksteps = 0;                      // 64-column steps of K
    int n_try = 0;                       // candidates below, in the order they are tried: the next one when a waiting grid cannot be resident
    int parts[MD_MAX_TRIES] = {0, 0, 0, 0, 0};
    int grid[MD_MAX_TRIES] = {0, 0, 0, 0, 0};
    int lds[MD_MAX_TRIES] = {0, 0, 0, 0, 0};
};
constexpr int GEMM_MID_N_FACTS = sizeof(GemmMidFacts) / sizeof(int), GEMM_MID_N_OUT = sizeof(GemmMidPlan) / sizeof(int);      // 18, 25

inline GemmMidPlan plan_gemm_mid(const GemmMidFacts &f)
{
    GemmMidPlan r;
    auto refuse = [&](int e) { r = GemmMidPlan(); r.error = e; return r; };
    const int rows[3] = {f.rows0, f.rows1, f.rows2};
    if (!f.mo) return refuse(GEMM_MID_ERR_LAYOUT);
    if (f.T < 1 || f.nsets < 1 || f.nsets > 3 || f.nblk < 8 || f.nblk % 4 != 0) return refuse(GEMM_MID_ERR_SHAPE);
    for (int i = 0; i < f.nsets; i++) if (rows[i] < 1 || rows[i] % 16 != 0) return refuse(GEMM_MID_ERR_ROWS);
    if (f.epi == GP_GLU && (f.nsets != 1 || !f.has_w1)) return refuse(GEMM_MID_ERR_GLU);
    if (f.ld_or % 8 != 0) return refuse(GEMM_MID_ERR_STRIDE);
    r.ta = f.ta == 8 ? 8 : 4;
    const int bm = 32 * r.ta, bne = f.epi == GP_GLU ? MD_BN / 2 : MD_BN;
    for (int i = 0; i < 3; i++) r.tile0[i + 1] = r.tile0[i] + (i < f.nsets ? (rows[i] + bne - 1) / bne : 0);
    r.tiles_n = r.tile0[f.nsets];
    for (int i = f.nsets; i < 3; i++) r.tile0[i] = 1 << 30;
    r.tiles_m = (f.T + bm - 1) / bm;
    r.ksteps = f.nblk * 32 / MD_BK;
    // parts of K: the most that still put ONE workgroup on a CU (the gated pair: two), every part >= min_steps steps
    const long long tiles = (long long)r.tiles_m * r.tiles_n, cap = ((f.two_per_cu || f.epi == GP_GLU) ? 2ll : 1ll) * f.num_cus;
    const bool may = !f.no_waits && f.waits_on && !(f.epi == GP_GLU && f.no_glu_split);
    const int mins = f.min_steps > 0 ? f.min_steps : 4;
    auto fits = [&](int ks) { return may && tiles * ks <= cap && r.ksteps / ks >= mins && (!f.max_parts || ks <= f.max_parts); };
    auto add = [&](int ks) { r.parts[r.n_try] = ks; r.grid[r.n_try] = (int)(tiles * ks); r.lds[r.n_try] = (int)md_lds_bytes(r.ta); r.n_try++; };
    if (r.ta == 4 && f.max_parts >= 16 && fits(16)) add(16);      // (16 parts: a measurement setting)
    if (fits(8)) add(8);
    if (fits(4)) add(4);
    if (fits(2)) add(2);
    add(1);
    return r;
}

// ------------------------------------------------------------------ k_gemm_big
constexpr int BIG_BK = 64;               // columns of a step (PF_BK)
enum GemmBigTilesBits {                  // ifa_gemm_big_tiles
    BIG_BIT_ON = 1, BIG_FORCE_SHIFT = 8, BIG_FORCE_MASK = 7,      // bits 8-10: 1 / 2 / 3 force 256 x 256 / 128 x 256 / 128 x 128, 4 / 5 / 6 the small tiles 64 x 64 / 128 x 64 / 64 x 128
    BIG_BIT_NO_SPLITK = 1 << 12, BIG_BIT_STREAM_K = 1 << 13,
};

// What the decision reads.  The order of the fields is the order of ifa_gemm_big_plan's `facts` array.
struct GemmBigFacts {
    int T = 0;
    int nsets = 1, rows0 = 0, rows1 = 0, rows2 = 0;
    int nblk = 0;                        // blocks per row
    int dtype = Q4_B32T1A;               // the format the kernel reads (its block capacity; F16: 32 columns count as a block)
    int epi = GP_PLAIN;
    int tiles_bits = 1;                  // ifa_gemm_big_tiles
    int num_cus = 0;
    int no_waits = 0, waits_on = 1;
    int has_w1 = 1, ld_or = 0;           // what gemm_big_ok reads besides: the gated pair's second matrix; ldy (or the three ldyset) | ldres where it is read
};
enum GemmBigPlanError {
    GEMM_BIG_OK = 0,
    GEMM_BIG_ERR_FORMAT = 1,             // blocks do not divide a 64-column step, or K is not whole steps
    GEMM_BIG_ERR_SHAPE = 2,              // T < 1, not 1..3 sets
    GEMM_BIG_ERR_EPILOGUE = 3,           // fused epilogues: Q4_B32T1A / B only
    GEMM_BIG_ERR_GLU = 4,                // the gated pair needs one set and W1
    GEMM_BIG_ERR_ROWS = 5,               // a set's rows % 8 != 0
    GEMM_BIG_ERR_STRIDE = 6,             // a stride % 8 != 0
};
struct GemmBigLaunch { int bm = 0, bn = 0, waves = 0, tn0 = 0, tn_count = 0, tiles_m = 0, lds = 0; };      // weight tiles [tn0, tn0 + tn_count) of bn rows (the gated pair: bn / 2 pairs)
// What a call runs.  The order of the fields is the order of ifa_gemm_big_plan's `out` array.
struct GemmBigPlan {
    int error = GEMM_BIG_OK;
    int pick = 0;                        // 1 .. 6: the tile shape chosen (the forced one, or the cheapest of 1 .. 3 by estimated rounds of the chip)
    int stream_k = 0;                    // bit 13 asked for it and the shape is eligible: tried first, the plan below when its grid cannot be resident
    int n_launch = 0;                    // 2: whole rounds of 256 x 256 tiles (full_n weight tiles), then rem_n tiles of 128 x 256 from tn0 = full_n
    GemmBigLaunch launch[2];
    int full_n = 0, rem_n = 0;
    int n_try = 0;                       // parts of K tried in order (128 x 128 tiles only; else {1})
    int ks[2] = {0, 0};
};
constexpr int GEMM_BIG_N_FACTS = sizeof(GemmBigFacts) / sizeof(int), GEMM_BIG_N_OUT = sizeof(GemmBigPlan) / sizeof(int);      // 14, 23

constexpr int big_lds_bytes(int bm, int bn) { return std::max(2 * (bm + bn) * (BIG_BK * 2), bm * (bn * 2 + 64)); }      // operand tiles; the epilogue's output tile

inline GemmBigPlan plan_gemm_big(const GemmBigFacts &f)
{
    GemmBigPlan r;
    auto refuse = [&](int e) { r = GemmBigPlan(); r.error = e; return r; };
    const int CAP = f.dtype == F16 ? 32 : block_capacity(f.dtype);
    const int rows[3] = {f.rows0, f.rows1, f.rows2};
    if (CAP <= 1 || BIG_BK % CAP != 0 || ((size_t)f.nblk * CAP) % BIG_BK != 0 || f.nblk < 1) return refuse(GEMM_BIG_ERR_FORMAT);
    if (f.T < 1 || f.nsets < 1 || f.nsets > 3) return refuse(GEMM_BIG_ERR_SHAPE);
    if (f.epi != GP_PLAIN && f.dtype != Q4_B32T1A && f.dtype != Q4_B32T1B) return refuse(GEMM_BIG_ERR_EPILOGUE);
    if (f.epi == GP_GLU && (f.nsets != 1 || !f.has_w1)) return refuse(GEMM_BIG_ERR_GLU);
    for (int i = 0; i < f.nsets; i++) if (rows[i] < 1 || rows[i] % 8 != 0) return refuse(GEMM_BIG_ERR_ROWS);
    if (f.ld_or % 8 != 0) return refuse(GEMM_BIG_ERR_STRIDE);
    const size_t T = (size_t)f.T, cus = (size_t)f.num_cus;
    auto cdiv = [](size_t a, size_t b) { return (a + b - 1) / b; };
    auto ntiles = [&](size_t bn) {
        const size_t bne = f.epi == GP_GLU ? bn / 2 : bn;
        size_t n = 0;
        for (int i = 0; i < f.nsets; i++) n += cdiv((size_t)rows[i], bne);
        return n;
    };
    auto set_launch = [&](int i, int bm, int bn, int waves, size_t tn0, size_t tn_count) {
        r.launch[i].bm = bm; r.launch[i].bn = bn; r.launch[i].waves = waves; r.launch[i].tn0 = (int)tn0; r.launch[i].tn_count = (int)tn_count;
        r.launch[i].tiles_m = (int)cdiv(T, (size_t)bm); r.launch[i].lds = big_lds_bytes(bm, bn);
        r.n_launch = i + 1;
    };
    const int force = (f.tiles_bits >> BIG_FORCE_SHIFT) & BIG_FORCE_MASK;
    auto rounds = [&](size_t bm, size_t bn, size_t per_cu) { return (double)cdiv(cdiv(T, bm) * ntiles(bn), cus * per_cu); };
    // 256 x 256: whole rounds of the chip; what is left of the last round goes to a second launch of 128-token tiles when those fit the
    // chip in one go
    const size_t tm256 = cdiv(T, 256), tn256 = ntiles(256), per_round = tm256 <= cus ? cus / tm256 : 0;
    const size_t full_n = per_round ? (tn256 / per_round) * per_round : 0, rem_n = tn256 - full_n;
    const bool split = full_n > 0 && rem_n > 0 && cdiv(T, 128) * rem_n <= cus && tm256 * rem_n < cus * 3 / 4;
    const size_t n128 = cdiv(T, 128) * ntiles(128);
    double c256 = CAP > 32 ? 1e30 : (split ? (double)(full_n / per_round) + 0.68 : rounds(256, 256, 1));   // (64-value blocks: the 256 x 256 variant would spill)
    const bool waits = !f.no_waits && f.waits_on;
    {   // stream-K (opt-in, bit 13): every CU takes floor(tiles / CUs) whole tiles and then an equal share of the K steps of the rest
        const size_t tiles = tm256 * tn256, S = (size_t)f.nblk * CAP / BIG_BK, rem = tiles % cus, share = rem * S / cus;
        const bool may_sk = !force && CAP <= 32 && (f.tiles_bits & BIG_BIT_STREAM_K) != 0 && waits && tiles * 4 >= cus * 3;
        if (may_sk && rem && share >= 20 && cdiv(S - 1, share) <= 3) {
            const double csk = (double)(tiles / cus) + (double)rem / (double)cus + 0.10;
            if (csk < c256) { c256 = csk; r.stream_k = 1; }
        }
    }
    const double c128x256 = rounds(128, 256, 1) * 0.68;
    const double c128 = n128 <= cus ? 0.41 : rounds(128, 128, 2) * 0.75;
    int pick = force;
    if (!pick) pick = (c256 <= c128x256 && c256 <= c128) ? 1 : (c128x256 <= c128 ? 2 : 3);
    r.pick = pick;
    r.n_try = 1; r.ks[0] = 1;
    if (pick == 4 && CAP <= 32) set_launch(0, 64, 64, 4, 0, ntiles(64));
    else if (pick == 5 && CAP <= 32) set_launch(0, 128, 64, 4, 0, ntiles(64));
    else if (pick == 6 && CAP <= 32) set_launch(0, 64, 128, 4, 0, ntiles(128));
    else if (pick == 1 && CAP <= 32) {
        if (split && !force) {
            set_launch(0, 256, 256, 8, 0, full_n);
            set_launch(1, 128, 256, 8, full_n, rem_n);
            r.full_n = (int)full_n; r.rem_n = (int)rem_n;
        } else set_launch(0, 256, 256, 8, 0, tn256);
    } else if (pick == 2 || pick == 1) set_launch(0, 128, 256, 8, 0, tn256);
    else {
        // 128 x 128 tiles that fill no more than one workgroup slot per CU (two fit): both halves of K at once -- only for products big
        // enough to matter (>= half the chip), never when a tile shape is forced.  One token tile (48 .. 128 tokens): four parts when that
        // still fits two workgroups per CU and a part keeps >= 1024 columns.  Eight waves per tile up to 512 tokens.
        const bool may_split = !force && f.epi != GP_GLU && (f.tiles_bits & BIG_BIT_NO_SPLITK) == 0 && waits;
        const size_t ksteps = (size_t)f.nblk * CAP / BIG_BK, K = (size_t)f.nblk * CAP;
        const bool splitk = may_split && n128 <= cus && n128 * 2 >= cus && ksteps % 2 == 0 && K >= 2048;
        const bool splitk4 = may_split && n128 * 2 < cus && n128 * 4 <= 2 * cus && ksteps % 4 == 0 && K >= 4096;
        const bool w8 = !force && T <= 512 && CAP <= 32;
        set_launch(0, 128, 128, w8 ? 8 : 4, 0, ntiles(128));
        if (splitk4) { r.ks[0] = 4; r.ks[1] = 1; r.n_try = 2; }
        else if (splitk) { r.ks[0] = 2; r.ks[1] = 1; r.n_try = 2; }
    }
    return r;
}

} // namespace ifa
