// ifa_kv_copy.hip -- rows [0, n_rows) of the K and V cache of every layer from one query slot to another (ifa_model_kv_copy): what
// the engine's prompt prefix cache (host/prefix_cache.h) needs when the slot that holds a prompt's leading rows is busy.
//
// One launch serves all 2 * layers segments: grid = (chunks of a segment) x (segments), the segments' addresses come from a device
// table of every slot's buffers (ifa_model::kvc_tab_dev).  2 * layers hipMemcpyAsync calls would move the same bytes with 2 * layers
// enqueues; a segment of a short prefix is a few hundred KiB, where the enqueue is what the copy costs.
//
// A workgroup is four wave64 and moves one 16 KiB chunk: every lane requests four independent 16-byte loads (256 lanes apart, so a
// wave's request is 1 KiB of consecutive bytes) before its first store -- 64 bytes in flight per lane, the copy has nothing else to
// hide the memory latency with.  A segment is n_rows * kv_row_bytes bytes, which is NOT always a multiple of 16 (a Q8_B32T2 row of
// kv_dim 128 is 136 bytes): the 16-byte body stops at the last whole piece and the last workgroup of the segment -- the
// one whose chunk is not whole -- moves the remaining < 16 bytes one per lane.  Nothing past n_rows * kv_row_bytes is written.  Both buffers start a hipMalloc allocation
// and the copy starts at row 0, so every 16-byte piece is aligned.
#include "ifa_engine_state.h"

namespace ifae {

static constexpr int KVC_THREADS = 256, KVC_LOADS = 4;
static constexpr size_t KVC_CHUNK16 = (size_t)KVC_THREADS * KVC_LOADS;      // 16-byte pieces per workgroup

typedef uint32_t kvc_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) kvc_u32x4 kvc_g16;      // (the table's pointers are global memory: global_load / _store, not flat)
typedef __attribute__((address_space(1))) uint8_t kvc_g1;

__global__ __launch_bounds__(KVC_THREADS) void k_kv_copy(void *const *src_tab, void *const *dst_tab, size_t bytes)
{
    const kvc_g1 *src = (const kvc_g1 *)src_tab[blockIdx.y];
    kvc_g1 *dst = (kvc_g1 *)dst_tab[blockIdx.y];
    const size_t n16 = bytes >> 4;
    const kvc_g16 *s16 = (const kvc_g16 *)src;
    kvc_g16 *d16 = (kvc_g16 *)dst;
    const size_t i0 = (size_t)blockIdx.x * KVC_CHUNK16 + threadIdx.x;
    if ((size_t)(blockIdx.x + 1) * KVC_CHUNK16 <= n16) {        // a whole chunk (uniform): the four loads leave before the first store
        kvc_u32x4 r[KVC_LOADS];
#pragma unroll
        for (int j = 0; j < KVC_LOADS; j++) r[j] = s16[i0 + (size_t)j * KVC_THREADS];
#pragma unroll
        for (int j = 0; j < KVC_LOADS; j++) d16[i0 + (size_t)j * KVC_THREADS] = r[j];
        return;
    }
    // the segment's last chunk: the remaining whole pieces, then the bytes behind the last of them
    for (size_t i = i0; i < n16; i += KVC_THREADS) d16[i] = s16[i];
    const size_t t = (n16 << 4) + threadIdx.x;
    if (t < bytes) dst[t] = src[t];
}

// the device table lists the buffers slots `a` and `b` have now; if not, a new table of all slots is staged on the model's stream
int kv_copy_table(ifa_model *m, int a, int b)
{
    const size_t L = m->layers.size(), n_slots = std::max<size_t>(m->slots.size(), 1);
    bool ok = m->kvc_tab.dev && m->kvc_tab_host.size() == n_slots * 2 * L;
    for (int slot : {a, b})
        for (size_t l = 0; ok && l < L; l++)
            ok = m->kvc_tab_host[((size_t)slot * L + l) * 2] == kv_ptr(m, l, slot, false)
                 && m->kvc_tab_host[((size_t)slot * L + l) * 2 + 1] == kv_ptr(m, l, slot, true);
    if (ok) return IFA_OK;
    if (m->kvc_tab.dev) m->kvc_retired.push_back(std::move(m->kvc_tab));
    m->kvc_tab_host.assign(n_slots * 2 * L, nullptr);
    for (size_t s = 0; s < n_slots; s++)
        for (size_t l = 0; l < L; l++) {
            m->kvc_tab_host[(s * L + l) * 2] = kv_ptr(m, l, (int)s, false);
            m->kvc_tab_host[(s * L + l) * 2 + 1] = kv_ptr(m, l, (int)s, true);
        }
    const size_t tab_bytes = m->kvc_tab_host.size() * sizeof(void *);
    hipError_t e = hipSuccess;
    if (m->kvc_tab.reserve(m->kvc_tab_host.size())) e = hipErrorOutOfMemory;
    else {
        memcpy(m->kvc_tab.pin, m->kvc_tab_host.data(), tab_bytes);
        // (the pinned block is never written again: it is valid for as long as this copy may be pending)
        e = hipMemcpyAsync(m->kvc_tab.dev, m->kvc_tab.pin, tab_bytes, hipMemcpyHostToDevice, m->stream);
    }
    if (e != hipSuccess) {
        m->kvc_tab_host.clear();          // (the next call builds the table again)
        return ifa_fail(IFA_ERR_HIP, "ifa_model_kv_copy: slot table of %zu bytes: %s", tab_bytes, hipGetErrorString(e));
    }
    return IFA_OK;
}

} // namespace ifae

extern "C" int ifa_model_kv_copy(ifa_model *m, int src_slot, int dst_slot, int n_rows)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_kv_copy: model not finalized");
    const int n_slots = std::max((int)m->slots.size(), 1);
    IFA_REQUIRE(src_slot >= 0 && src_slot < n_slots, "ifa_model_kv_copy: source slot %d of %d", src_slot, n_slots);
    IFA_REQUIRE(dst_slot >= 0 && dst_slot < n_slots, "ifa_model_kv_copy: destination slot %d of %d", dst_slot, n_slots);
    IFA_REQUIRE(src_slot != dst_slot, "ifa_model_kv_copy: source and destination are both slot %d", src_slot);
    IFA_REQUIRE(n_rows >= 0 && n_rows <= m->cfg.max_ctx, "ifa_model_kv_copy: %d rows (max_ctx %d)", n_rows, m->cfg.max_ctx);
    if (n_rows == 0 || m->layers.empty()) return IFA_OK;
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    IFA_HIP_CHECK(hipStreamIsCapturing(m->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return ifa_fail(IFA_ERR_STATE, "ifa_model_kv_copy: the model's stream is being captured");
    int rc = kv_copy_table(m, src_slot, dst_slot);
    if (rc) return rc;
    const size_t L = m->layers.size(), bytes = (size_t)n_rows * m->kv_row_bytes;
    // (+ 1 piece: a segment that ends on a chunk boundary, or holds fewer than 16 bytes, still gets the workgroup that moves the tail)
    const unsigned chunks = ifa_cdiv((bytes >> 4) + 1, KVC_CHUNK16);
    k_kv_copy<<<dim3(chunks, (unsigned)(2 * L)), dim3(KVC_THREADS), 0, m->stream>>>(m->kvc_tab.dev + (size_t)src_slot * 2 * L,
                                                                                 m->kvc_tab.dev + (size_t)dst_slot * 2 * L, bytes);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}
