// ifa_gemm_rows_plan.h -- what a rows GEMM launch runs (k_gemm_rows_mfma: ifa_gemm_rows_mfma.hip for the tiled layout, ifa_gemm_rows_mo.hip
// for the MO layout): refusal, rows staged, tiles per workgroup, grid, chunk form and count, LDS bytes, and the attempts in the order they
// are tried -- K parts first where they apply, then the plain launch -- as a pure host function: no HIP calls, nothing of GmArgs.  The
// launchers (gemm_rows_mfma_launch, gemm_rows_mo_launch) take their run-time values from the plan and their template arguments from the
// same constants; the C ABI exposes it for tests (ifa_gemm_rows_plan), and the launcher records what it ran (ifa_gemm_rows_launches).
// The measurements behind every number are in the launchers' comments and in DESIGN.md.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ifa {

// ------------------------------------------------------------------ geometry constants (GmGeo, ifa_gemm_rows_mfma_body.h, is built from these)
constexpr int GM_THREADS = 512, GM_WAVES = 8;
constexpr int gm_chunk_cols(int cs) { return cs * 128; }                  // cs = supersteps (128 columns) per LDS chunk of the activation rows: 32 or 16
constexpr int gm_row_stride(int cs) { return gm_chunk_cols(cs) * 2 + 16; }  // bytes per activation row in LDS (+16: conflict-free 16-byte reads)
constexpr int gm_bpw(int cs) { return cs * 4 / GM_WAVES; }                // blocks of a chunk per wave and row: 16 or 8
constexpr int gm_patch_bytes(int cs) { return 16 * (gm_bpw(cs) * 16 + 16) + 16 * (gm_bpw(cs) * 4 + 16); }      // tiled layout: a wave's LDS patch (codes, words)
constexpr int GM_WHOLE_LDS_MAX = 150 * 1024, GM_WHOLE_K_MAX = 16384;      // whole-row staging (CH = 2)
constexpr int gm_tx_tiled(int T) { return T <= 2 ? 2 : (T <= 4 ? 4 : (T <= 8 ? 8 : 16)); }
constexpr int gm_tx_mo(int T) { return T <= 16 ? gm_tx_tiled(T) : 32; }
constexpr size_t gm_parts_bytes(int maxt) { return (size_t)maxt * GM_WAVES * 256 * 4; }      // the waves' partial 16 x 16 tiles
// whole-row staging (CH == 2): tx rows of K columns
constexpr size_t gm_smem_whole(int tx, int K, int maxt) { return std::max((size_t)tx * ((size_t)K * 2 + 16), gm_parts_bytes(maxt)); }
constexpr size_t gm_smem(int T, int maxt, int mo)
{
    if (mo && gm_tx_mo(T) == 32) return std::max((size_t)32 * gm_row_stride(16), 2 * gm_parts_bytes(maxt));
    if (mo) return std::max((size_t)gm_tx_mo(T) * gm_row_stride(32) + (size_t)16 * GM_WAVES * 4, gm_parts_bytes(maxt));
    const int cs = gm_tx_tiled(T) > 8 ? 16 : 32;
    return std::max((size_t)gm_tx_tiled(T) * gm_row_stride(cs) + (size_t)GM_WAVES * gm_patch_bytes(cs) + 8 * GM_WAVES * 4, gm_parts_bytes(maxt));      // + the norm's group sums
}

inline int gm_tiles_per_workgroup(int ntiles, int grid_cap, bool pairs, int *wgs);      // (below)

enum GemmRowsEpilogue { GR_PLAIN = 0, GR_RESIDUAL = 1, GR_GLU = 2 };      // == GmEpilogue (ifa_gemm_rows_mfma.h)

// What the decision reads.  The order of the fields is the order of ifa_gemm_rows_plan's `facts` array.
struct GemmRowsFacts {
    int T = 0;
    int nsets = 1, rows0 = 0, rows1 = 0, rows2 = 0;      // weight rows of each set (the gated pair: rows of w1 = rows of w3)
    int nblk = 0;                        // 32-weight blocks per row (K / 32)
    int epi = GR_PLAIN;
    int norm = 0;                        // 1: the RMS norm while the rows are staged
    int mo = 0;                          // GmArgs::mo: the weights are MO copies
    int has_w1 = 1;                      // the gated pair's second matrix is there
    int no_waits = 0;                    // GmArgs::no_waits: the caller's veto of launches that wait
    int waits_on = 1;                    // waits_enabled() (ifa_host.h)
    int num_cus = 0, visible_cus = 0;    // of the device; the CUs this process can occupy
    // the settings (0 = the default; rows_settings, ifa_gemm_rows_mfma.hip, fills them from the environment once)
    int wgs_per_cu = 0;                  // IFA_ROWS_WGS_PER_CU: workgroups per CU the grid may have at <= 8 rows (default 1)
    int kparts_off = 0;                  // IFA_ROWS_KPARTS_OFF: never K parts
    int kparts_min = 0;                  // IFA_ROWS_KPARTS_MIN: least chunks of K for K parts (default 2)
};
enum GemmRowsPlanError {
    GEMM_ROWS_OK = 0,
    GEMM_ROWS_ERR_SHAPE = 1,             // T outside 2..16 (MO: 2..32), K not whole 128-column supersteps, not 1..3 sets
    GEMM_ROWS_ERR_NORM = 2,              // the norm prologue needs the whole row in one chunk (K <= 4096) and <= 8 rows (MO: <= 16)
    GEMM_ROWS_ERR_GLU = 3,               // the gated pair needs one set and W1
    GEMM_ROWS_ERR_ROWS = 4,              // a set without rows; several sets: a set's rows % 16 != 0
    GEMM_ROWS_ERR_OFFSET = 5,            // a matrix whose byte offsets pass 32 bits
    GEMM_ROWS_ERR_NO_KERNEL = 6,         // no instance for this epilogue / norm: residual behind the norm prologue; tiled layout: the gated pair
                                         // without the norm at <= 8 rows; an epilogue or norm the kernel does not have
};
// One attempt.  kparts 0: the plain launch (every workgroup walks all of K for its tiles).
struct GemmRowsTry {
    int kparts = 0;                      // workgroups that share a tile group, each with its own chunks of K
    int kpm = 0;                         // the instance's KPM: tiles a workgroup finishes (= the plain launch's tiles per workgroup: 1 or 2)
    int tiles = 0;                       // tiles per workgroup = the instance's MAXT (K parts: tiles per group, kpm x kparts)
    int groups = 0;                      // tile groups (plain: the workgroups)
    int grid = 0;                        // workgroups
    int lds = 0;                         // dynamic LDS bytes
    int scratch = 0;                     // bytes of the fp32 sums the parts exchange (8-byte granules)
};
constexpr int GEMM_ROWS_MAX_TRIES = 2;
// What a launch runs.  The order of the fields is the order of ifa_gemm_rows_plan's `out` array.
struct GemmRowsPlan {
    int error = GEMM_ROWS_OK;
    int total_rows = 0, ntiles = 0;      // virtual rows of all sets; their 16-row tiles
    int tx = 0;                          // activation rows staged (the instance's TX): 2, 4, 8, 16, 32
    int ch = 0;                          // the instance's CH: 1 one chunk, 0 the chunk loop, 2 whole rows
    int chunk_cols = 0, nchunk = 0;      // columns of an LDS chunk of the activation rows; chunks of K
    int n_try = 0;                       // attempts below, in the order they are tried: the next one when a waiting grid cannot be resident
    GemmRowsTry tries[GEMM_ROWS_MAX_TRIES];
};
constexpr int GEMM_ROWS_N_FACTS = sizeof(GemmRowsFacts) / sizeof(int), GEMM_ROWS_N_OUT = sizeof(GemmRowsPlan) / sizeof(int);      // 17, 22
constexpr int GEMM_ROWS_N_TRY = sizeof(GemmRowsTry) / sizeof(int);      // 7

inline GemmRowsPlan plan_gemm_rows(const GemmRowsFacts &f)
{
    GemmRowsPlan r;
    auto refuse = [&](int e) { r = GemmRowsPlan(); r.error = e; return r; };
    const int rows[3] = {f.rows0, f.rows1, f.rows2};
    const int T = f.T, K = f.nblk * 32, epi = f.epi, norm = f.norm;
    // ---- gemm_rows_mfma_fused_ok
    if (T < 2 || T > (f.mo ? 32 : 16) || f.nblk <= 0 || f.nblk % 4 != 0 || f.nsets < 1 || f.nsets > 3) return refuse(GEMM_ROWS_ERR_SHAPE);      // (17..32 rows: MO layout only)
    if (norm == 1 && (K > gm_chunk_cols(32) || T > (f.mo ? 16 : 8))) return refuse(GEMM_ROWS_ERR_NORM);      // whole rows in one chunk (tiled layout: <= 8 rows)
    if (epi == GR_GLU && (f.nsets != 1 || !f.has_w1)) return refuse(GEMM_ROWS_ERR_GLU);
    for (int i = 0; i < f.nsets; i++) if (rows[i] <= 0 || (f.nsets > 1 && rows[i] % 16 != 0)) return refuse(GEMM_ROWS_ERR_ROWS);
    for (int i = 0; i < f.nsets; i++)      // 32-bit byte offsets inside a matrix (tiled and MO copies are 20 bytes per block + padding)
        if (((size_t)rows[i] + 16) * ((size_t)f.nblk + 16) * 20 >= ((size_t)1 << 32)) return refuse(GEMM_ROWS_ERR_OFFSET);
    // ---- the instances that exist
    r.tx = f.mo ? gm_tx_mo(T) : gm_tx_tiled(T);
    const bool one = f.mo && K <= gm_chunk_cols(32) && T <= 16;      // (the tiled kernels are always the chunk loop)
    {
        bool have = (epi == GR_PLAIN || epi == GR_RESIDUAL) && norm == 0;
        if (f.mo) {
            if (one) have = have || (epi == GR_PLAIN && norm == 1) || (epi == GR_GLU && (norm == 0 || norm == 1));
            else have = have || (epi == GR_GLU && norm == 0);
        } else {
            if (r.tx <= 8) have = have || ((epi == GR_PLAIN || epi == GR_GLU) && norm == 1);
            else have = have || (epi == GR_GLU && norm == 0);
        }
        if (!have) return refuse(GEMM_ROWS_ERR_NO_KERNEL);
    }
    // ---- tiles per workgroup and grid (gm_tiles_per_workgroup): one workgroup per CU; 1, 2, 3, 4, 6 or 8 tiles each; past 8 they queue
    for (int i = 0; i < f.nsets; i++) r.total_rows += rows[i];
    const int ntiles = r.ntiles = (r.total_rows + 15) / 16;
    const int grid_cap = f.num_cus * (T <= 8 ? std::max(1, f.wgs_per_cu) : 1);
    int wgs = 0;
    const int maxt = gm_tiles_per_workgroup(ntiles, grid_cap, epi == GR_GLU, &wgs);
    r.chunk_cols = gm_chunk_cols(f.mo ? (T <= 16 ? 32 : 16) : (r.tx > 8 ? 16 : 32));
    r.nchunk = (K + r.chunk_cols - 1) / r.chunk_cols;
    auto add = [&](int kparts, int kpm, int tiles, int groups, int grid, size_t lds, size_t scratch) {
        GemmRowsTry &t = r.tries[r.n_try++];
        t.kparts = kparts; t.kpm = kpm; t.tiles = tiles; t.groups = groups; t.grid = grid; t.lds = (int)lds; t.scratch = (int)scratch;
    };
    if (!f.mo) { r.ch = 0; add(0, 0, maxt, wgs, wgs, gm_smem(T, maxt, 0), 0); return r; }
    // ---- MO layout: 2..4 rows longer than one chunk, no norm: staged whole (CH = 2)
    if (!one && norm == 0 && T <= 4 && K <= GM_WHOLE_K_MAX && (epi == GR_PLAIN || epi == GR_RESIDUAL) && gm_smem_whole(T <= 2 ? 2 : 4, K, maxt) <= (size_t)GM_WHOLE_LDS_MAX) {
        r.ch = 2; add(0, 0, maxt, wgs, wgs, gm_smem_whole(T <= 2 ? 2 : 4, K, maxt), 0);
        return r;
    }
    r.ch = one ? 1 : 0;
    // ---- K parts: 9..32 rows walking two chunks or more, one or two tiles per workgroup before.  kparts = the most parts that divide the
    // chunk count, leave an instance (2, 3, 4, 6, 8 tiles per group) and keep every workgroup of every group resident at once
    const int kparts_min = f.kparts_min > 0 ? f.kparts_min : 2;
    if (!one && norm == 0 && (epi == GR_PLAIN || epi == GR_RESIDUAL) && T >= 9 && !f.kparts_off && !f.no_waits && f.waits_on && (maxt == 1 || maxt == 2)) {
        int kparts = 0;
        for (int d = std::min(r.nchunk, 8 / maxt); d >= 2 && r.nchunk >= kparts_min; d--) {
            if (r.nchunk % d != 0 || maxt * d == 5 || maxt * d == 7) continue;
            if ((ntiles + maxt * d - 1) / (maxt * d) * d > std::min(f.num_cus, f.visible_cus)) continue;
            kparts = d; break;
        }
        if (kparts >= 2) {
            const int tiles = maxt * kparts, groups = (ntiles + tiles - 1) / tiles, ntc = T > 16 ? 2 : 1;
            add(kparts, maxt, tiles, groups, groups * kparts, gm_smem(T, tiles, 1), (size_t)groups * tiles * kparts * ntc * 256 * 8);
        }
    }
    add(0, 0, maxt, wgs, wgs, gm_smem(T, maxt, 1), 0);
    return r;
}

// ------------------------------------------------------------------ what the launcher ran (ifa_gemm_rows_launches)
// Plain data, one copy per launch; the order of the fields is the order of the ints of a record in ifa_gemm_rows_launches' `out` array.
struct GemmRowsLaunchRecord {
    int T = 0, total_rows = 0, nblk = 0, epi = 0, norm = 0, mo = 0;
    int tx = 0, ch = 0, nchunk = 0;
    int n_try = 0, attempt = 0;          // attempts the plan listed; the index of the one that ran
    GemmRowsTry ran;
    // attempt > 0: what wait_grid_fits saw when it declined attempt 0 (all 0 when attempt == 0)
    int declined_grid = 0, occupancy = 0, visible_cus = 0, waits_on = 0, err_word = 0;
};
constexpr int GEMM_ROWS_N_RECORD = sizeof(GemmRowsLaunchRecord) / sizeof(int), GEMM_ROWS_RECORDS = 8;      // 23 ints; the last 8 launches
constexpr int GEMM_ROWS_COUNT_MAX = 0x7fffffff;
// The ring behind ifa_gemm_rows_launches: the slot of the next record stays in 0 .. 7 and the count of launches since the last read
// saturates, so a process that never reads (every production process) can launch for ever.  Plain data; the caller serialises.
struct GemmRowsLaunchRing {
    GemmRowsLaunchRecord rec[GEMM_ROWS_RECORDS];
    int head = 0;                        // slot the next record goes to
    int count = 0;                       // launches since the last read (GEMM_ROWS_COUNT_MAX: that many or more)
    void push(const GemmRowsLaunchRecord &r)
    {
        rec[head] = r;
        head = (head + 1) % GEMM_ROWS_RECORDS;
        if (count < GEMM_ROWS_COUNT_MAX) count++;
    }
    // out[0] = records that follow (oldest first), out[1] = launches since the last read, then the records; clears
    void take(int *out, int n_out)
    {
        const int room = n_out >= 2 ? (n_out - 2) / GEMM_ROWS_N_RECORD : 0, n = std::min(std::min(count, GEMM_ROWS_RECORDS), room);
        out[0] = n; out[1] = count;
        for (int i = 0; i < n; i++) {
            const GemmRowsLaunchRecord &r = rec[(head + GEMM_ROWS_RECORDS - n + i) % GEMM_ROWS_RECORDS];
            const int *src = reinterpret_cast<const int *>(&r);
            for (int k = 0; k < GEMM_ROWS_N_RECORD; k++) out[2 + i * GEMM_ROWS_N_RECORD + k] = src[k];
        }
        head = 0; count = 0;
    }
};
// tiles per workgroup of ntiles 16-row tiles on at most grid_cap workgroups: 1, 2, 3, 4, 6 or 8 (5 -> 6, 7 -> 8; past 8 the workgroups
// queue); pairs: the gated pair's tiles come as 1 .. 4 pairs of (W1, W3) tiles, the result counts both.  *wgs: the workgroups
inline int gm_tiles_per_workgroup(int ntiles, int grid_cap, bool pairs, int *wgs)
{
    int w = std::min(grid_cap, ntiles);
    int mt = (ntiles + w - 1) / w;
    if (mt > 8) { mt = 8; w = (ntiles + 7) / 8; }                // (more workgroups than CUs: they queue)
    if (mt == 5) mt = 6;
    if (mt == 7) mt = 8;
    if (pairs) {                               // pairs of tiles: 1, 2, 3, 4 pairs per workgroup
        if (mt > 4) { mt = 4; w = (ntiles + 3) / 4; }
        mt = mt == 3 ? 6 : mt * 2;
    }
    *wgs = w;
    return mt;
}

} // namespace ifa
