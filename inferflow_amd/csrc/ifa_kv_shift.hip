// ifa_kv_shift.hip -- context shift on the device (ifa_model_kv_shift, ifa_kv_shift_rows): of the n_rows cache rows of one query
// slot the rows [keep, keep + discard) are dropped, the rows behind them move down by `discard` rows, and the moved K rows -- stored
// with RoPE applied -- are rotated back by `discard` positions on the way: R(p) k becomes R(-discard) R(p) k = R(p - discard) k.  V
// rows, and K rows of a model without RoPE, move byte for byte.  Rows [0, keep) and every byte from row n_rows - discard on are not
// written.  Arithmetic: DESIGN.md "Context shift"; tests/kv_shift_util.py is its numpy model, bit for bit.
//
// One launch serves all 2 * layers segments, like k_kv_copy: grid = (chunks of a segment) x (segments), addresses from the slot
// table (ifa_model::kvc_tab).  A launch's source and destination ranges are DISJOINT: when the moved rows outnumber the dropped
// ones the host issues ascending pieces of `discard` rows on the model's stream, each piece's destination a range the piece before
// it has consumed.  (The engine's policy drops at least as many rows as it moves: one launch.)
//
// The unit of work is one kv head's slice of one row -- head_dim halves (F16) or head_dim / 32 blocks of 34 bytes (Q8_B32T2): the
// rotation's pairs and the quantiser's blocks never leave it, and the moved range is a whole number of consecutive units.  A
// workgroup takes KVS_UNITS = 64 of them, so a chunk starts at a multiple of 64 * unit bytes -- a multiple of 16 whatever the row
// size -- and the access width of a launch follows from the byte offsets of its source and destination (and, for ifa_kv_shift_rows, from the
// alignment of the caller's buffers) alone: 16-byte vectors
// where both allow them (every F16 model with whole 8-half rows), else 8 / 4 / 2.  No access is issued at an address that is not a
// multiple of its size; the < width bytes behind a chunk's last whole piece move one byte per lane.
//   move segments (V; K without RoPE): pieces through registers, four loads in flight per lane before the first store.
//   rotating segments: the chunk is staged in LDS, rotated there with the call's (cos, sin) table -- head_dim / 2 pairs, computed
//   once per call, never per element -- and written out.  Q8 rows are dequantised into a second LDS block of halves, rotated, and
//   the blocks that hold a rotated column are requantised with the store quantiser of k_draft_kv_store, expression for expression;
//   a block without one keeps its bytes (requantising is not idempotent).
#include "ifa_engine_state.h"

namespace ifae {

static constexpr int KVS_THREADS = 256, KVS_UNITS = 64, KVS_LOADS = 4;

typedef __attribute__((address_space(1))) uint8_t kvs_g1;
template <int W> struct kvs_vec;
template <> struct kvs_vec<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <> struct kvs_vec<8> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct kvs_vec<4> { typedef uint32_t type; };
template <> struct kvs_vec<2> { typedef uint16_t type; };

struct KvShiftParams {
    void *const *tab;          // [2 * layers] K, V buffers of the slot; null: the two pointers below (one layer)
    void *k0, *v0;             // either may be null: that side is skipped
    const float *rot;          // [head_dim / 2] (cos, sin) of the rotation by -discard positions
    size_t src_off, dst_off;   // bytes from the buffer's start
    size_t n_units;            // kv-head slices to move (rows * kv_heads)
    int unit_bytes, head_dim, q8, rope_order, rope_cols;
};

// grid (chunks, segments).  Dynamic LDS: KVS_UNITS * unit_bytes, + KVS_UNITS * head_dim halves with a Q8 cache.
template <int W>
__global__ __launch_bounds__(KVS_THREADS) void k_kv_shift(const KvShiftParams P)
{
    typedef typename kvs_vec<W>::type vec_t;
    typedef __attribute__((address_space(1))) vec_t gvec_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t kvs_lds[];
    const int seg = blockIdx.y, tid = threadIdx.x;
    void *basep = P.tab ? P.tab[seg] : (seg == 0 ? P.k0 : P.v0);
    if (!basep) return;                                               // (uniform)
    const size_t u0 = (size_t)blockIdx.x * KVS_UNITS;
    const int units = (int)min((size_t)KVS_UNITS, P.n_units - u0);
    const size_t bytes = (size_t)units * P.unit_bytes, off = u0 * (size_t)P.unit_bytes;
    const kvs_g1 *src = (const kvs_g1 *)basep + P.src_off + off;
    kvs_g1 *dst = (kvs_g1 *)basep + P.dst_off + off;
    const gvec_t *sv = (const gvec_t *)src;
    gvec_t *dv = (gvec_t *)dst;
    const size_t nv = bytes / W;
    const bool rotate = (seg & 1) == 0 && P.rope_order != 0;         // (uniform) even segments are K
    if (!rotate) {
        for (size_t i0 = tid; i0 < nv; i0 += (size_t)KVS_THREADS * KVS_LOADS) {
            vec_t r[KVS_LOADS];
#pragma unroll
            for (int j = 0; j < KVS_LOADS; j++) { const size_t i = i0 + (size_t)j * KVS_THREADS; if (i < nv) r[j] = sv[i]; }
#pragma unroll
            for (int j = 0; j < KVS_LOADS; j++) { const size_t i = i0 + (size_t)j * KVS_THREADS; if (i < nv) dv[i] = r[j]; }
        }
        const size_t t = nv * W + tid;
        if (t < bytes) dst[t] = src[t];
        return;
    }
    // ---- stage
    vec_t *lv = reinterpret_cast<vec_t *>(kvs_lds);
    for (size_t i = tid; i < nv; i += KVS_THREADS) lv[i] = sv[i];
    { const size_t t = nv * W + tid; if (t < bytes) kvs_lds[t] = src[t]; }
    __syncthreads();
    const int HD = P.head_dim, ub = P.unit_bytes;
    half_t *hb = P.q8 ? reinterpret_cast<half_t *>(kvs_lds + (size_t)KVS_UNITS * ub) : reinterpret_cast<half_t *>(kvs_lds);
    const int hstride = P.q8 ? HD : ub / 2;                          // halves from one unit to the next
    if (P.q8) {      // v = f16(float(scale) * float(code))
        for (int j = tid; j < units * HD; j += KVS_THREADS) {
            const int u = j / HD, d = j - u * HD;
            const uint8_t *blk = kvs_lds + (size_t)u * ub + (size_t)(d >> 5) * 34;
            const half_t sc = __builtin_bit_cast(half_t, (uint16_t)(blk[0] | (blk[1] << 8)));
            hb[j] = f2h(__fmul_rn(h2f(sc), (float)(int8_t)blk[2 + (d & 31)]));
        }
        __syncthreads();
    }
    // ---- rotate: the expressions of rope_apply, every product, the difference and the sum rounded on their own
    const int HP = HD / 2;
    for (int j = tid; j < units * HP; j += KVS_THREADS) {
        const int u = j / HP, col = j - u * HP;
        int i0, i1;
        if (P.rope_order == 2) { if (2 * col >= P.rope_cols) continue; i0 = col; i1 = col + P.rope_cols / 2; }
        else { i0 = 2 * col; i1 = 2 * col + 1; }
        const float c = P.rot[2 * col], s = P.rot[2 * col + 1];
        half_t *row = hb + (size_t)u * hstride;
        const float x0 = h2f(row[i0]), x1 = h2f(row[i1]);
        row[i0] = f2h(__fsub_rn(__fmul_rn(x0, c), __fmul_rn(x1, s)));
        row[i1] = f2h(__fadd_rn(__fmul_rn(x0, s), __fmul_rn(x1, c)));
    }
    __syncthreads();
    if (P.q8) {      // one 32-value block per half wave; the loop count is the same for every lane of a wave
        const int NB = HD / 32, nblk = units * NB, lane = tid & 63, wave = tid >> 6, l32 = lane & 31;
        for (int b0 = wave * 2; b0 < nblk; b0 += 2 * (KVS_THREADS / 64)) {
            const int b = b0 + (lane >> 5);
            const bool live = b < nblk;
            const int bc = live ? b : nblk - 1, u = bc / NB, bb = bc - u * NB;
            const float val = h2f(hb[(size_t)u * HD + bb * 32 + l32]);
            const float mx = half_wave_max(fabsf(val));
            const float sc = mx / 127;
            int qv = sc <= 0.000001f ? 0 : (int)roundf(val / sc);
            qv = min(max(qv, -128), 127);
            const bool rotated = P.rope_order != 2 || bb * 32 < P.rope_cols;      // a block without a rotated column keeps its bytes
            if (live && rotated) {
                uint8_t *blk = kvs_lds + (size_t)u * ub + (size_t)bb * 34;
                blk[2 + l32] = (uint8_t)(int8_t)qv;
                if (l32 == 0) { const uint16_t sb = f2hbits(sc); blk[0] = (uint8_t)(sb & 0xff); blk[1] = (uint8_t)(sb >> 8); }
            }
        }
        __syncthreads();
    }
    // ---- store
    for (size_t i = tid; i < nv; i += KVS_THREADS) dv[i] = lv[i];
    { const size_t t = nv * W + tid; if (t < bytes) dst[t] = kvs_lds[t]; }
}

// (cos, -sin) of position `discard`, from the rope_angle the steps' own tables come from
__global__ void k_kv_shift_table(float *rot, int half_dim, int pos, float theta, int rope_dims)
{
    for (int c = threadIdx.x; c < half_dim; c += blockDim.x) {
        float cs, sn;
        rope_angle(c, pos, theta, rope_dims, cs, sn);
        rot[2 * c] = cs; rot[2 * c + 1] = -sn;
    }
}

// the launches of one call: one if the moved rows do not outnumber the dropped ones, else ascending pieces of `discard` rows
static int kv_shift_launches(KvShiftParams P, int segments, size_t row_bytes, size_t kv_heads, size_t keep, size_t discard, size_t n_rows,
                             hipStream_t s, size_t base_align = 0)
{
    const size_t moved = n_rows - keep - discard;
    const size_t lds = (size_t)KVS_UNITS * P.unit_bytes + (P.q8 ? (size_t)KVS_UNITS * P.head_dim * 2 : 0);
    for (size_t r0 = 0; r0 < moved; r0 += discard) {
        const size_t rows = std::min(discard, moved - r0);
        P.src_off = (keep + discard + r0) * row_bytes; P.dst_off = (keep + r0) * row_bytes;
        P.n_units = rows * kv_heads;
        const dim3 grid(ifa_cdiv(P.n_units, KVS_UNITS), (unsigned)segments), block(KVS_THREADS);
        // (a chunk is a multiple of 16 bytes; base_align: the low address bits of caller-supplied buffers -- the slots' own start an allocation)
        const size_t a = P.src_off | P.dst_off | base_align;
        if (a % 16 == 0) k_kv_shift<16><<<grid, block, lds, s>>>(P);
        else if (a % 8 == 0) k_kv_shift<8><<<grid, block, lds, s>>>(P);
        else if (a % 4 == 0) k_kv_shift<4><<<grid, block, lds, s>>>(P);
        else k_kv_shift<2><<<grid, block, lds, s>>>(P);      // (a unit is a whole number of halves or of 34-byte blocks: every offset is even)
        IFA_LAUNCH_CHECK();
    }
    return IFA_OK;
}

static int kv_shift_geometry(const char *who, int kv_dtype, size_t kv_heads, size_t head_dim, int rope_order, int rope_cols, size_t keep,
                             size_t discard, size_t n_rows, KvShiftParams &P, size_t &row_bytes)
{
    IFA_REQUIRE(kv_dtype == F16 || kv_dtype == Q8_B32T2, "%s: cache type %d (F16 or Q8_B32T2)", who, kv_dtype);
    IFA_REQUIRE(kv_heads >= 1 && head_dim >= 2 && head_dim <= 128 && head_dim % 2 == 0, "%s: %zu kv heads of %zu", who, kv_heads, head_dim);
    const bool q8 = kv_dtype == Q8_B32T2;
    IFA_REQUIRE(!q8 || head_dim % 32 == 0, "%s: Q8 cache with head_dim %zu (whole 32-blocks only)", who, head_dim);
    IFA_REQUIRE(discard >= 1, "%s: discard %zu rows (at least 1)", who, discard);
    IFA_REQUIRE(keep + discard <= n_rows, "%s: keep %zu + discard %zu exceed the %zu rows", who, keep, discard, n_rows);
    IFA_REQUIRE(rope_order >= 0 && rope_order <= 2, "%s: rope_order %d", who, rope_order);
    IFA_REQUIRE(rope_order != 2 || (rope_cols >= 0 && rope_cols <= (int)head_dim && rope_cols % 2 == 0), "%s: rope_cols %d of head_dim %zu", who,
                rope_cols, head_dim);
    P.unit_bytes = q8 ? (int)(head_dim / 32) * 34 : (int)head_dim * 2;
    P.head_dim = (int)head_dim; P.q8 = q8 ? 1 : 0; P.rope_order = rope_order; P.rope_cols = rope_cols;
    row_bytes = kv_heads * (size_t)P.unit_bytes;
    return IFA_OK;
}

} // namespace ifae

extern "C" int ifa_kv_shift_rows(int kv_dtype, void *kcache, void *vcache, size_t kv_heads, size_t head_dim, int rope_order, int rope_cols,
                                 const float *table_dev, size_t keep, size_t discard, size_t n_rows, ifa_stream stream)
{
    KvShiftParams P = {};
    size_t row_bytes = 0;
    int rc = kv_shift_geometry("ifa_kv_shift_rows", kv_dtype, kv_heads, head_dim, rope_order, rope_cols, keep, discard, n_rows, P, row_bytes);
    if (rc) return rc;
    IFA_REQUIRE(rope_order == 0 || !kcache || table_dev, "ifa_kv_shift_rows: null table");
    const size_t base_align = ((size_t)(uintptr_t)kcache | (size_t)(uintptr_t)vcache) & 15;
    IFA_REQUIRE(base_align % 2 == 0, "ifa_kv_shift_rows: cache pointers %p / %p are not 2-byte aligned", kcache, vcache);
    P.k0 = kcache; P.v0 = vcache; P.rot = table_dev;
    if (!kcache && !vcache) return IFA_OK;
    return kv_shift_launches(P, 2, row_bytes, kv_heads, keep, discard, n_rows, ifa_s(stream), base_align);
}

extern "C" int ifa_model_kv_shift(ifa_model *m, int slot, int keep, int discard, int n_rows)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_kv_shift: model not finalized");
    const int n_slots = std::max((int)m->slots.size(), 1);
    IFA_REQUIRE(slot >= 0 && slot < n_slots, "ifa_model_kv_shift: slot %d of %d", slot, n_slots);
    IFA_REQUIRE(keep >= 0, "ifa_model_kv_shift: keep %d rows", keep);
    IFA_REQUIRE(discard >= 1, "ifa_model_kv_shift: discard %d rows (at least 1)", discard);
    IFA_REQUIRE(n_rows >= 0 && n_rows <= m->cfg.max_ctx, "ifa_model_kv_shift: %d rows (max_ctx %d)", n_rows, m->cfg.max_ctx);
    IFA_REQUIRE((long long)keep + discard <= n_rows, "ifa_model_kv_shift: keep %d + discard %d exceed the %d rows", keep, discard, n_rows);
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "ifa_model_kv_shift: partitioned workers have no context shift");
    const ifa_model_config &c = m->cfg;
    const int rope_cols = (int)(c.head_dim * c.partial_rotary + 0.5f);
    KvShiftParams P = {};
    size_t row_bytes = 0;
    int rc = kv_shift_geometry("ifa_model_kv_shift", c.kv_dtype, (size_t)c.kv_heads, (size_t)c.head_dim, c.rope_order, rope_cols, (size_t)keep,
                               (size_t)discard, (size_t)n_rows, P, row_bytes);
    if (rc) return rc;
    if (row_bytes != m->kv_row_bytes) return ifa_fail(IFA_ERR_STATE, "ifa_model_kv_shift: cache rows of %zu bytes, expected %zu", m->kv_row_bytes, row_bytes);
    if (m->layers.empty() || keep + discard == n_rows) return IFA_OK;      // (nothing behind the dropped rows)
    IFA_HIP_CHECK(hipSetDevice(c.device));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    IFA_HIP_CHECK(hipStreamIsCapturing(m->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return ifa_fail(IFA_ERR_STATE, "ifa_model_kv_shift: the model's stream is being captured");
    rc = kv_copy_table(m, slot, slot);
    if (rc) return rc;
    if (c.rope_order != 0) {
        if (!m->kvs_rot && (rc = m->kvs_rot.alloc((size_t)c.head_dim)) != 0) return rc;
        k_kv_shift_table<<<1, 64, 0, m->stream>>>(m->kvs_rot, c.head_dim / 2, discard, c.rope_theta, rope_cols);
        IFA_LAUNCH_CHECK();
    }
    const size_t L = m->layers.size();
    P.tab = m->kvc_tab.dev + (size_t)slot * 2 * L; P.rot = m->kvs_rot;
    return kv_shift_launches(P, (int)(2 * L), row_bytes, (size_t)c.kv_heads, (size_t)keep, (size_t)discard, (size_t)n_rows, m->stream);
}
