// ifa_engine.hip -- per-device decode worker, model life cycle (see ifa_engine_state.h for the layout of the worker's units):
// tensors in (reference layout + the re-tiled / MFMA-operand-order copies), KV caches and query slots, options, debug buffers.
#include <mutex>
#include <unordered_map>
#include "ifa_engine_state.h"

// ------------------------------------------------ the two memory spaces of the worker's buffers (ifa_buf_hip.h)
namespace ifa {

namespace {
struct SpaceBook {
    std::mutex mu;
    std::unordered_map<void *, size_t> live;      // what the two spaces have handed out and not taken back
    long long live_bytes = 0, fail_at = 0;        // fail_at: the n-th allocation from now fails once (ifa_debug_alloc_fail_at; 0: off)
};
SpaceBook &book() { static SpaceBook *b = new SpaceBook(); return *b; }      // (never destroyed: buffers may go at process exit)

template <class Alloc> int space_alloc(const char *call, void **p, size_t bytes, Alloc alloc)
{
    SpaceBook &b = book();
    *p = nullptr;
    {
        std::lock_guard<std::mutex> g(b.mu);
        if (b.fail_at > 0 && --b.fail_at == 0)
            return ifa_fail(IFA_ERR_HIP, "%s(%zu bytes) failed: out of memory (simulated: ifa_debug_alloc_fail_at)", call, bytes);
    }
    const hipError_t e = alloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return ifa_fail(IFA_ERR_HIP, "%s(%zu bytes) failed: %s", call, bytes, hipGetErrorString(e));
    }
    if (*p) { std::lock_guard<std::mutex> g(b.mu); b.live[*p] = bytes; b.live_bytes += (long long)bytes; }
    return IFA_OK;
}

void space_forget(void *p)
{
    SpaceBook &b = book();
    std::lock_guard<std::mutex> g(b.mu);
    auto it = b.live.find(p);
    if (it != b.live.end()) { b.live_bytes -= (long long)it->second; b.live.erase(it); }
}
} // namespace

int DevSpace::alloc(void **p, size_t bytes) { return space_alloc("hipMalloc", p, bytes, [](void **q, size_t n) { return hipMalloc(q, n); }); }
void DevSpace::free(void *p) { space_forget(p); (void)hipFree(p); }
int PinSpace::alloc(void **p, size_t bytes) { return space_alloc("hipHostMalloc", p, bytes, [](void **q, size_t n) { return hipHostMalloc(q, n, hipHostMallocDefault); }); }
void PinSpace::free(void *p) { space_forget(p); (void)hipHostFree(p); }

} // namespace ifa

extern "C" int ifa_debug_alloc_fail_at(long long nth)
{
    IFA_REQUIRE(nth >= 0, "ifa_debug_alloc_fail_at: nth %lld", nth);
    std::lock_guard<std::mutex> g(book().mu);
    book().fail_at = nth;
    return IFA_OK;
}

extern "C" int ifa_debug_live_allocs(long long *count, long long *bytes)
{
    std::lock_guard<std::mutex> g(book().mu);
    if (count) *count = (long long)book().live.size();
    if (bytes) *bytes = book().live_bytes;
    return IFA_OK;
}

namespace ifae {

int perf_begin(ifa_model *m, int key)
{
    if (!m->opt_perf_stat) return -1;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(m->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return -1; }
    auto take = [&]() -> hipEvent_t {
        if (!m->perf_pool.empty()) { hipEvent_t e = m->perf_pool.back(); m->perf_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return e;
    };
    ifa_model::PerfSpanRec r; r.key = key; r.e0 = take(); r.e1 = take();
    if (!r.e0 || !r.e1) { if (r.e0) m->perf_pool.push_back(r.e0); if (r.e1) m->perf_pool.push_back(r.e1); return -1; }
    if (hipEventRecord(r.e0, m->stream) != hipSuccess) { (void)hipGetLastError(); m->perf_pool.push_back(r.e0); m->perf_pool.push_back(r.e1); return -1; }
    m->perf_spans.push_back(r);
    return (int)m->perf_spans.size() - 1;
}

void perf_end(ifa_model *m, int idx)
{
    if (idx < 0 || idx >= (int)m->perf_spans.size()) return;
    if (hipEventRecord(m->perf_spans[(size_t)idx].e1, m->stream) != hipSuccess) (void)hipGetLastError();
}

// the stream is drained, every span's milliseconds are ADDED to its key (UpdatePerfStat's rule: iter->second += value)
int perf_collect(ifa_model *m)
{
    if (m->perf_spans.empty()) return IFA_OK;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    for (auto &r : m->perf_spans) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) m->perf_map[r.key] += ms;
        else (void)hipGetLastError();
        m->perf_pool.push_back(r.e0); m->perf_pool.push_back(r.e1);
    }
    m->perf_spans.clear();
    return IFA_OK;
}

void drop_graphs(ifa_model *m)
{
    if (m->tp_graph_exec) { (void)hipGraphExecDestroy(m->tp_graph_exec); m->tp_graph_exec = nullptr; }
    if (m->tp_graph) { (void)hipGraphDestroy(m->tp_graph); m->tp_graph = nullptr; }
    if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
    if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
    if (m->graph_exec_n) { (void)hipGraphExecDestroy(m->graph_exec_n); m->graph_exec_n = nullptr; }
    if (m->graph_n) { (void)hipGraphDestroy(m->graph_n); m->graph_n = nullptr; }
    for (auto &sl : m->slots) {
        if (sl.exec) { (void)hipGraphExecDestroy(sl.exec); sl.exec = nullptr; }
        if (sl.graph) { (void)hipGraphDestroy(sl.graph); sl.graph = nullptr; }
    }
    for (auto &kv : m->batch_graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
    m->batch_graphs.clear();
    for (auto &kv : m->draft_graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
    m->draft_graphs.clear();
    for (auto &kv : m->fed_graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
    m->fed_graphs.clear();
    sampled_drop_graphs(m);
}

// ------------------------------------------------ op-by-op forward (any T)
// All or nothing: the new set is built aside and installed only when every allocation has succeeded; a failure leaves the model as
// it was (old buffers, old scratch_tokens, captured steps valid).  The transient peak is the old set plus the new one.
int ensure_scratch(ifa_model *m, int T)
{
    if (T <= m->scratch_tokens) return IFA_OK;
    const ifa_model_config &c = m->cfg;
    const size_t D = c.dim, QD = (size_t)c.heads * c.head_dim, KVD = (size_t)c.kv_heads * c.head_dim, F = c.ffn;
    size_t maxcols = std::max(std::max(D, QD), F);
    Scratch n;
    int rc;
    if ((rc = n.x.alloc(T * D)) || (rc = n.x2.alloc(T * D)) || (rc = n.xn.alloc(T * D)) || (rc = n.hn.alloc(T * D)) || (rc = n.pn.alloc(T * D))
        || (rc = n.q.alloc(T * QD)) || (rc = n.k.alloc(T * KVD)) || (rc = n.v.alloc(T * KVD)) || (rc = n.att.alloc(T * QD))
        || (rc = n.a.alloc(T * D)) || (rc = n.f.alloc(T * D)) || (rc = n.t1.alloc(std::max<size_t>(T, 3) * F)) || (rc = n.t2.alloc(T * F))
        || (rc = n.logits.alloc((size_t)T * c.vocab)))
        return rc;
    if (!m->dqkv && (rc = n.dqkv.alloc(QD + 2 * KVD))) return rc;
    if (T <= 32 && !m->bqkv && ((rc = n.bqkv.alloc(32 * (QD + 2 * KVD))) || (rc = n.brope.alloc(32 * (size_t)c.head_dim)))) return rc;
    if (c.experts > 0) {
        const size_t cap = (size_t)T * (size_t)std::max(1, c.moe_top_k);
        if ((rc = n.moe_gate.alloc((size_t)T * c.experts)) || (rc = n.moe_out.alloc((size_t)T * D)) || (rc = n.moe_in.alloc((size_t)T * D))
            || (rc = n.moe_wdev.alloc(cap)) || (rc = n.moe_idx.alloc(cap)) || (rc = n.moe_pin.alloc(cap * (sizeof(int) + 2) + 16)))
            return rc;
        if (!m->moe_route) {
            if ((rc = n.moe_route.alloc(64 / sizeof(int)))) return rc;
            IFA_HIP_CHECK(hipMemsetAsync(n.moe_route, 0, 64, m->stream));
        }
        // device-routed path: every expert's rows at once (cap entries)
        if ((rc = n.moe_sel.alloc(cap)) || (rc = n.moe_epos.alloc(cap)) || (rc = n.moe_counts.alloc(16))
            || (rc = n.moe_xq_in.alloc(cap * (D / 32 + 1) * 34)) || (rc = n.moe_xq_mid.alloc(cap * (F / 32 + 1) * 34))
            || (rc = n.moe_tiles.alloc((cap / 64 + (size_t)c.experts + 1) * sizeof(MoeTile)))
            || (rc = n.moe_singles.alloc(((size_t)c.experts + 1) * sizeof(MoeSingle))) || (rc = n.moe_smalls.alloc(((size_t)c.experts + 1) * sizeof(MoeTile)))
            || (rc = n.moe_selw.alloc(cap)) || (rc = n.moe_g1.alloc(cap * F)) || (rc = n.moe_g3.alloc(cap * F)) || (rc = n.moe_gin.alloc(cap * D))
            || (rc = n.moe_gout.alloc(cap * D)))
            return rc;
    }
    if ((rc = n.xq.alloc((maxcols / 32 + 1) * 34))) return rc;
    if (!m->attq && (rc = n.attq.alloc(xq_image_bytes(c.heads * c.head_dim)))) return rc;
    if ((rc = n.tokens_dev.alloc((size_t)T))) return rc;
    // commit (nothing below fails): what did not grow keeps its block -- captured steps and moe_route's zeroes live at those addresses
    if (!n.dqkv) n.dqkv = std::move(m->dqkv);
    if (!n.bqkv) { n.bqkv = std::move(m->bqkv); n.brope = std::move(m->brope); }
    if (!n.moe_route) n.moe_route = std::move(m->moe_route);
    if (!n.attq) n.attq = std::move(m->attq);
    static_cast<Scratch &>(*m) = std::move(n);
    m->scratch_tokens = T;
    // buffers moved: any captured graph is stale
    drop_graphs(m);
    return IFA_OK;
}

void *kv_ptr(ifa_model *m, size_t layer, int slot, bool is_v)
{
    if (slot == m->cur_slot || m->slots.empty()) return is_v ? m->layers[layer].vcache : m->layers[layer].kcache;
    const ifa_model::KvSlot &sl = m->slots[(size_t)slot];
    return is_v ? sl.v[layer] : sl.k[layer];
}

// (a failed allocation -- the copies are 4.3 GB for Llama-2-7B Q4 -- is not an error of the step that triggered it: every partial
//  copy is dropped, opt_rows_mo goes off and the tiled kernels (<= 16 rows per launch) serve the batched steps)
int ensure_mo(ifa_model *m)
{
    if (!m->opt_rows_mo) return IFA_OK;
    // (option "debug_mo_alloc_fail": the build reports an allocation failure after its first copy -- the tests' way to walk the downgrade)
    const int rc = ensure_mo_build(m);
    if (rc == IFA_OK) return IFA_OK;
    (void)hipGetLastError();
    for (Layer &L : m->layers) {
        for (Tensor &t : L.t) t.mo.reset();
        for (Tensor &t : L.experts) t.mo.reset();
        L.moe_table_mo.reset();
    }
    m->opt_rows_mo = 0;
    drop_graphs(m);
    fprintf(stderr, "inferflow_amd: the rows GEMM's operand-order weight copies could not be built (%s); batched steps use the tiled kernels\n", ifa_last_error());
    return IFA_OK;
}

int ensure_mo_build(ifa_model *m)
{
    const ifa_model_config &c = m->cfg;
    bool built = false;
    for (Layer &L : m->layers) {
        const bool moe = c.experts > 0 && L.t[T_MOE_GATE].present();
        const int ids[] = {T_WQ, T_WK, T_WV, T_WO, T_W1, T_W3, T_W2};
        for (int id : ids) {
            Tensor &t = L.t[id];
            if (moe && (id == T_W1 || id == T_W3 || id == T_W2)) continue;
            if (t.mo || !t.present() || !t.tiled || !rows_mo_fmt(t.dtype) || t.cols % 128 != 0) continue;
            if (m->opt_debug_mo_alloc_fail && built) return ifa_fail(IFA_ERR_HIP, "hipMalloc: out of memory (simulated: debug_mo_alloc_fail)");
            int rc = t.mo.alloc(gemm_rows_mo_bytes(t.rows, t.cols));
            if (rc) return rc;
            rc = gemm_rows_mo_build(t.dtype, t.tiled, t.rows, t.cols, t.mo, m->stream);
            if (rc) return rc;
            built = true;
        }
    }
    // mixture-of-experts layers: the experts' matrices too, with their pointer table {w1, w3, w2, -} (the order of moe_table):
    // the experts that collect 2..8 rows of a batched step take the grouped MO launches (moe_ffn_device)
    for (Layer &L : m->layers) {
        if (!(c.experts > 0 && L.t[T_MOE_GATE].present()) || L.moe_table_mo || (int)L.experts.size() != c.experts * 3) continue;
        bool ok = true;
        for (Tensor &t : L.experts) ok = ok && t.present() && t.tiled && is_q4(t.dtype) && t.cols % 128 == 0;
        if (!ok) continue;
        std::vector<void *> tab((size_t)c.experts * 4, nullptr);
        for (int e = 0; e < c.experts; e++) {
            const int order[3] = {0, 2, 1};                       // experts[e * 3 + {0, 1, 2}] = w1, w2, w3
            for (int k = 0; k < 3; k++) {
                Tensor &t = L.experts[(size_t)e * 3 + order[k]];
                if (!t.mo) {
                    int rc = t.mo.alloc(gemm_rows_mo_bytes(t.rows, t.cols));
                    if (rc) return rc;
                    rc = gemm_rows_mo_build(t.dtype, t.tiled, t.rows, t.cols, t.mo, m->stream);
                    if (rc) return rc;
                    built = true;
                }
                tab[(size_t)e * 4 + k] = t.mo;
            }
        }
        { int rc = L.moe_table_mo.alloc(tab.size()); if (rc) return rc; }
        IFA_HIP_CHECK(hipMemcpy(L.moe_table_mo, tab.data(), tab.size() * sizeof(void *), hipMemcpyHostToDevice));
    }
    if (built) IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return IFA_OK;
}

// Long prompts of a model in a 64-weight nibble format: Q4_B32T1A-layout copies of the dense layers' matrices for k_gemm_big
int ensure_x32(ifa_model *m)
{
    bool built = false;
    for (Layer &L : m->layers) {
        const int ids[] = {T_WQ, T_WK, T_WV, T_WO, T_W1, T_W3, T_W2};
        for (int id : ids) {
            Tensor &t = L.t[id];
            if (t.x32 || !t.present() || !t.tiled || (t.dtype != Q4_B64T1 && t.dtype != Q3H_B64T1) || t.cols % 64 != 0) continue;
            int rc = t.x32.alloc(t.rows * (t.cols / 32) * 20);
            if (rc) return rc;
            rc = expand_b64_to_q4b32(t.dtype, t.tiled, t.rows, t.cols, t.x32, m->stream);
            if (rc) return rc;
            built = true;
        }
    }
    if (built) IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return IFA_OK;
}

// option q3h_native: the 32-byte-per-block streaming copies of the Q3H_B64T1 matrices the k_dec_gemv launches of a dense layer read
// (Wo, W1, W3, W2), built on the first decode call with the option on
int ensure_q3hn(ifa_model *m)
{
    bool built = false;
    for (Layer &L : m->layers) {
        const int ids[] = {T_WO, T_W1, T_W3, T_W2};
        for (int id : ids) {
            Tensor &t = L.t[id];
            if (t.q3hn || !t.present() || t.dtype != Q3H_B64T1 || t.cols % 64 != 0) continue;
            int rc = t.q3hn.alloc(t.rows * (t.cols / 64) * 32);
            if (rc) return rc;
            rc = q3h_native_rows(t.data, t.rows, t.cols, t.q3hn, m->stream);
            if (rc) return rc;
            built = true;
        }
    }
    if (built) IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return IFA_OK;
}

} // namespace ifae

extern "C" {

int ifa_model_create(const ifa_model_config *cfg, ifa_model **out)
{
    IFA_REQUIRE(cfg && out, "ifa_model_create: null pointer");
    IFA_REQUIRE(cfg->dim > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->kv_heads > 0 && cfg->head_dim > 0
                && cfg->vocab > 0 && cfg->max_ctx > 0, "ifa_model_create: bad hyper-parameters");
    IFA_REQUIRE(cfg->heads % cfg->kv_heads == 0, "ifa_model_create: heads %d not a multiple of kv_heads %d", cfg->heads, cfg->kv_heads);
    IFA_REQUIRE(cfg->kv_dtype == F16 || cfg->kv_dtype == Q8_B32T2, "ifa_model_create: kv dtype %d", cfg->kv_dtype);
    IFA_REQUIRE(cfg->norm_kind == 0 || cfg->norm_kind == 1, "ifa_model_create: norm_kind %d", cfg->norm_kind);
    IFA_HIP_CHECK(hipSetDevice(cfg->device));
    ifa_model *m = new ifa_model();
    m->cfg = *cfg;
    if (m->cfg.eps <= 0) m->cfg.eps = 1e-5f;
    if (m->cfg.kq_scale <= 0) m->cfg.kq_scale = 1.0f;
    if (m->cfg.partial_rotary <= 0) m->cfg.partial_rotary = 1.0f;
    if (m->cfg.tp_size <= 0) m->cfg.tp_size = 1;
    for (float *sc : {&m->cfg.attn_out_scale, &m->cfg.ffn_out_scale, &m->cfg.out_scale}) if (*sc <= 0.0f) *sc = 1.0f;
    if (m->cfg.embd_scale < 0.0f) m->cfg.embd_scale = sqrtf((float)m->cfg.dim);      // LinearNorm's default scale (tensor_opr.cu:492-494)
    m->layers.resize((size_t)cfg->layers);
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete m; return ifa_fail(IFA_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    *out = m;
    return IFA_OK;
}

int ifa_model_destroy(ifa_model *m)
{
    if (!m) return IFA_OK;
    (void)hipSetDevice(m->cfg.device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    drop_graphs(m);
    if (m->stream) (void)ifa_gemm_release_stream((ifa_stream)m->stream);
    // every buffer goes with its owner, on the current device and behind the synchronisation above; then what has no owner
    const hipStream_t stream = m->own_stream ? m->stream : nullptr, side = m->side_stream;
    std::vector<hipEvent_t> events;
    events.swap(m->perf_pool);
    for (auto &r : m->perf_spans) { events.push_back(r.e0); events.push_back(r.e1); }
    delete m;
    if (stream) (void)hipStreamDestroy(stream);
    if (side) (void)hipStreamDestroy(side);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    return IFA_OK;
}

int ifa_model_set_tensor(ifa_model *m, int layer, int tensor_id, int expert, int dtype, const void *dev_src,
                         size_t rows, size_t cols)
{
    IFA_REQUIRE(m && dev_src, "ifa_model_set_tensor: null pointer");
    IFA_REQUIRE(tensor_id >= 0 && tensor_id < T_MAX, "ifa_model_set_tensor: tensor id %d", tensor_id);
    IFA_REQUIRE(expert < 0 || (expert < m->cfg.experts && layer >= 0 && (tensor_id == T_W1 || tensor_id == T_W2 || tensor_id == T_W3)),
                "ifa_model_set_tensor: expert %d (of %d) / tensor %d", expert, m->cfg.experts, tensor_id);
    IFA_REQUIRE(block_capacity(dtype) > 0 && dtype != F32 && dtype != Q3H_NATIVE, "ifa_model_set_tensor: dtype %d", dtype);
    IFA_REQUIRE(cols % (size_t)block_capacity(dtype) == 0, "ifa_model_set_tensor: cols %zu vs block capacity", cols);
    {   // the scratch buffers are sized from the config and the kernels are launched with the tensor's dimensions: a
        // mismatch would write out of bounds on the device, so it is refused here (per-shard dimensions under TP)
        const ifa_model_config &c = m->cfg;
        const size_t D = (size_t)c.dim, QD = (size_t)c.heads * c.head_dim, KVD = (size_t)c.kv_heads * c.head_dim, F = (size_t)c.ffn;
        size_t er = 0, ec = 0;        // expected rows / cols; 0 = free
        bool vec = false;             // [1][n] vectors (norm weights, biases) may also arrive as [n][1]
        switch (tensor_id) {
        case T_EMBD: ec = D; break;
        case T_LM_HEAD: ec = D; break;                      // rows: the vocabulary (or this rank's shard of it)
        case T_OUT_NORM: case T_OUT_NORM_B: case T_ATTN_NORM: case T_ATTN_NORM_B: case T_FFN_NORM: case T_FFN_NORM_B:
        case T_WO_B: case T_W2_B: vec = true; ec = D; break;
        case T_WQ: er = QD; ec = D; break;
        case T_WK: case T_WV: er = KVD; ec = D; break;
        case T_WO: er = D; ec = QD; break;
        case T_W1: case T_W3: er = F; ec = D; break;
        case T_W2: er = D; ec = F; break;
        case T_MOE_GATE: er = (size_t)c.experts; ec = D; break;
        case T_WQ_B: vec = true; ec = QD; break;
        case T_WK_B: case T_WV_B: vec = true; ec = KVD; break;
        case T_W1_B: case T_W3_B: vec = true; ec = F; break;
        default: break;
        }
        if (vec) IFA_REQUIRE(rows * cols == ec, "ifa_model_set_tensor: tensor %d holds %zu x %zu values, the model needs %zu", tensor_id, rows, cols, ec);
        else {
            IFA_REQUIRE(ec == 0 || cols == ec, "ifa_model_set_tensor: tensor %d has %zu columns, the model needs %zu", tensor_id, cols, ec);
            IFA_REQUIRE(er == 0 || rows == er, "ifa_model_set_tensor: tensor %d has %zu rows, the model needs %zu", tensor_id, rows, er);
        }
        if (tensor_id == T_LM_HEAD && layer < 0) IFA_REQUIRE(rows <= (size_t)c.vocab, "ifa_model_set_tensor: lm_head has %zu rows, vocab is %d", rows, c.vocab);
        if (tensor_id == T_EMBD) IFA_REQUIRE(rows <= (size_t)c.vocab, "ifa_model_set_tensor: %zu embedding rows, vocab is %d", rows, c.vocab);
    }
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    Tensor *t;
    if (tensor_id < 10) t = &m->g[tensor_id];
    else {
        IFA_REQUIRE(layer >= 0 && layer < m->cfg.layers, "ifa_model_set_tensor: layer %d", layer);
        Layer &L = m->layers[(size_t)layer];
        if (expert >= 0) {
            if (L.experts.empty()) L.experts.resize((size_t)m->cfg.experts * 3);
            t = &L.experts[(size_t)expert * 3 + (tensor_id == T_W1 ? 0 : (tensor_id == T_W2 ? 1 : 2))];
        } else t = &L.t[tensor_id];
    }
    *t = Tensor();
    if (expert >= 0) m->layers[(size_t)layer].moe_table_mo.reset();      // it points into the copy just freed: ensure_mo rebuilds it
    // load time: the source may have been produced on another stream (e.g. the caller's default stream)
    IFA_HIP_CHECK(hipDeviceSynchronize());
    const size_t bytes = rows * ifa_row_bytes(dtype, cols);
    int rc = t->data.alloc(bytes);
    if (rc) return rc;
    IFA_HIP_CHECK(hipMemcpyAsync(t->data, dev_src, bytes, hipMemcpyDeviceToDevice, m->stream));
    t->dtype = dtype; t->rows = rows; t->cols = cols;
    const bool is_matrix = (layer < 0 && tensor_id == T_LM_HEAD) || tensor_id == T_WQ || tensor_id == T_WK || tensor_id == T_WV || tensor_id == T_WO
        || tensor_id == T_W1 || tensor_id == T_W2 || tensor_id == T_W3;
    if (is_matrix && ax8_eligible(dtype)) {
        if ((rc = t->tiled.alloc(rows * ifa_tiled_row_bytes(dtype, cols)))) return rc;
        rc = ifa_repack_weights(dtype, t->data, rows, cols, t->tiled, m->stream);
        if (rc) return rc;
    }
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    drop_graphs(m);
    return IFA_OK;
}

int ifa_model_set_tensor_f16(ifa_model *m, int layer, int tensor_id, int expert, int target_dtype,
                             const void *dev_src_f16, size_t rows, size_t cols)
{
    IFA_REQUIRE(m && dev_src_f16, "ifa_model_set_tensor_f16: null pointer");
    if (target_dtype == F16) return ifa_model_set_tensor(m, layer, tensor_id, expert, F16, dev_src_f16, rows, cols);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    DevBuf<void> tmp;
    const size_t bytes = rows * ifa_row_bytes(target_dtype, cols);
    IFA_REQUIRE(bytes > 0, "ifa_model_set_tensor_f16: dtype %d", target_dtype);
    int rc = tmp.alloc(bytes);
    if (rc) return rc;
    IFA_HIP_CHECK(hipDeviceSynchronize());   // source may come from another stream
    rc = ifa_quantize(target_dtype, dev_src_f16, rows, cols, tmp, m->stream);   // DeviceTensorBuilder::Build_Quant
    if (rc == IFA_OK) rc = ifa_model_set_tensor(m, layer, tensor_id, expert, target_dtype, tmp, rows, cols);
    (void)hipStreamSynchronize(m->stream);      // (tmp goes behind the copy out of it)
    return rc;
}

int ifa_model_finalize(ifa_model *m)
{
    IFA_REQUIRE(m, "ifa_model_finalize: null model");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    (void)wait_err_word();       // (the device's wait-error word exists before any step can be captured: ifa_host.h)
    const ifa_model_config &c = m->cfg;
    const size_t KVD = (size_t)c.kv_heads * c.head_dim;
    IFA_REQUIRE(c.kv_dtype != Q8_B32T2 || KVD % 32 == 0, "Q8 KV cache needs kv_dim %% 32 == 0");
    m->kv_row_bytes = ifa_row_bytes(c.kv_dtype, KVD);
    int rc;
    for (Layer &L : m->layers) {
        if (!L.kcache) {   // KVCache::Init (kv_cache.cc:278-319): (kv_dim, max_ctx) per layer
            // (at least DEC_ATTN_MIN_ROWS rows are allocated: the fused attention kernel requests its first 256 rows unclamped)
            const size_t kv_alloc = m->kv_row_bytes * (size_t)std::max(c.max_ctx, DEC_ATTN_MIN_ROWS);
            if ((rc = L.kcache.alloc(kv_alloc)) || (rc = L.vcache.alloc(kv_alloc))) return rc;
            IFA_HIP_CHECK(hipMemsetAsync(L.kcache, 0, kv_alloc, m->stream));
            IFA_HIP_CHECK(hipMemsetAsync(L.vcache, 0, kv_alloc, m->stream));
        }
        if (c.experts > 0 && (int)L.experts.size() == c.experts * 3) {      // pointer table for the fused MoE kernels
            std::vector<void *> tab((size_t)c.experts * 4, nullptr);
            for (int e = 0; e < c.experts; e++) {
                tab[(size_t)e * 4 + 0] = L.experts[(size_t)e * 3 + 0].tiled;
                tab[(size_t)e * 4 + 1] = L.experts[(size_t)e * 3 + 2].tiled;
                tab[(size_t)e * 4 + 2] = L.experts[(size_t)e * 3 + 1].tiled;
            }
            if (!L.moe_table && (rc = L.moe_table.alloc(tab.size()))) return rc;
            IFA_HIP_CHECK(hipMemcpy(L.moe_table, tab.data(), tab.size() * sizeof(void *), hipMemcpyHostToDevice));
            std::vector<void *> aos((size_t)c.experts * 3, nullptr);
            for (int e = 0; e < c.experts; e++) for (int k3 = 0; k3 < 3; k3++) aos[(size_t)e * 3 + k3] = L.experts[(size_t)e * 3 + k3].data;
            if (!L.moe_table_aos && (rc = L.moe_table_aos.alloc(aos.size()))) return rc;
            IFA_HIP_CHECK(hipMemcpy(L.moe_table_aos, aos.data(), aos.size() * sizeof(void *), hipMemcpyHostToDevice));
        }
    }
    if (!m->attn_ws.S) {
        if ((rc = m->attn_ws_S.alloc((size_t)c.heads * c.max_ctx + 32))      // (+ 64 bytes: the last row is read in whole 16-byte pieces)
            || (rc = m->attn_ws_lmax.alloc((size_t)c.heads * DEC_ATTN_MAX_SPLITS))
            || (rc = m->attn_ws_opart.alloc((size_t)c.heads * DEC_ATTN_MAX_SPLITS * c.head_dim))) return rc;
        m->attn_ws.S = m->attn_ws_S; m->attn_ws.lmax = m->attn_ws_lmax; m->attn_ws.opart = m->attn_ws_opart;
    }
    if (!m->state) {
        if ((rc = m->state.alloc(8 + ifa_model::RING))) return rc;
        IFA_HIP_CHECK(hipMemsetAsync(m->state, 0, sizeof(int) * (8 + ifa_model::RING), m->stream));
        if ((rc = m->rope_tab.alloc((size_t)c.head_dim)) || (rc = m->host_pinned.alloc(16 + ifa_model::RING))) return rc;
    }
    if ((rc = ensure_scratch(m, 1))) return rc;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    m->finalized = true;
    return IFA_OK;
}

int ifa_model_reset(ifa_model *m)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_reset: model not finalized");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    for (Layer &L : m->layers) {
        IFA_HIP_CHECK(hipMemsetAsync(L.kcache, 0, m->kv_row_bytes * (size_t)m->cfg.max_ctx, m->stream));
        IFA_HIP_CHECK(hipMemsetAsync(L.vcache, 0, m->kv_row_bytes * (size_t)m->cfg.max_ctx, m->stream));
    }
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return IFA_OK;
}

int ifa_model_kv_slots(ifa_model *m, int n_slots)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_kv_slots: model not finalized");
    IFA_REQUIRE(n_slots >= 1 && n_slots <= 4096, "ifa_model_kv_slots: n_slots %d", n_slots);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    if (m->slots.empty()) m->slots.resize(1);        // slot 0 = the cache finalize() made (active, nothing parked)
    IFA_REQUIRE((int)m->slots.size() <= n_slots, "ifa_model_kv_slots: cannot shrink below %zu slots", m->slots.size());
    const size_t bytes = m->kv_row_bytes * (size_t)std::max(m->cfg.max_ctx, DEC_ATTN_MIN_ROWS);
    while ((int)m->slots.size() < n_slots) {
        ifa_model::KvSlot sl;      // pushed only when complete: a failure drops what it holds (behind the memsets: freeing waits for the device)
        for (size_t l = 0; l < m->layers.size(); l++) {
            DevBuf<void> k, v;
            int rc;
            if ((rc = k.alloc(bytes)) || (rc = v.alloc(bytes))) return rc;
            IFA_HIP_CHECK(hipMemsetAsync(k, 0, bytes, m->stream));
            IFA_HIP_CHECK(hipMemsetAsync(v, 0, bytes, m->stream));
            sl.k.push_back(std::move(k)); sl.v.push_back(std::move(v));
        }
        m->slots.push_back(std::move(sl));
    }
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return IFA_OK;
}

int ifa_model_select_kv(ifa_model *m, int slot)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_select_kv: model not finalized");
    if (m->slots.empty()) m->slots.resize(1);
    IFA_REQUIRE(slot >= 0 && slot < (int)m->slots.size(), "ifa_model_select_kv: slot %d of %zu", slot, m->slots.size());
    if (slot == m->cur_slot) return IFA_OK;
    // the captured multi-GPU step holds the outgoing slot's cache pointers
    if (m->tp_graph_exec) { (void)hipGraphExecDestroy(m->tp_graph_exec); m->tp_graph_exec = nullptr; }
    if (m->tp_graph) { (void)hipGraphDestroy(m->tp_graph); m->tp_graph = nullptr; }
    ifa_model::KvSlot &out = m->slots[(size_t)m->cur_slot], &in = m->slots[(size_t)slot];
    out.k.clear(); out.v.clear();
    for (Layer &L : m->layers) { out.k.push_back(std::move(L.kcache)); out.v.push_back(std::move(L.vcache)); }
    out.graph = m->graph; out.exec = m->graph_exec;
    if (m->graph_exec_n) { (void)hipGraphExecDestroy(m->graph_exec_n); m->graph_exec_n = nullptr; }      // (the multi-step replay is not kept per slot)
    if (m->graph_n) { (void)hipGraphDestroy(m->graph_n); m->graph_n = nullptr; }
    for (size_t l = 0; l < m->layers.size(); l++) { m->layers[l].kcache = std::move(in.k[l]); m->layers[l].vcache = std::move(in.v[l]); }
    m->graph = in.graph; m->graph_exec = in.exec;
    in.k.clear(); in.v.clear(); in.graph = nullptr; in.exec = nullptr;
    m->cur_slot = slot;
    return IFA_OK;
}

int ifa_model_set_option(ifa_model *m, const char *name, int value)
{
    IFA_REQUIRE(m && name, "ifa_model_set_option: null pointer");
    if (strcmp(name, "pool_lse") == 0) { m->opt_pool_lse = value != 0; return IFA_OK; }      // (nothing captured depends on it: the graphs stay)
    struct { const char *n; int *p; } opts[] = {
        {"fused", &m->opt_fused}, {"graph", &m->opt_graph}, {"rpw_qkv", &m->opt_rpw_qkv}, {"rpw_wo", &m->opt_rpw_wo},
        {"rpw_ffn", &m->opt_rpw_ffn}, {"rpw_w2", &m->opt_rpw_w2}, {"rpw_lm", &m->opt_rpw_lm}, {"trace", &m->opt_trace},
        {"bench_mode", &m->opt_bench_mode}, {"touch_stride", &m->opt_touch_stride}, {"time_pos", &m->opt_time_pos}, {"attn_split_ctx", &m->opt_attn_split_ctx}, {"batch_graph", &m->opt_batch_graph}, {"gemm_rows", &m->opt_gemm_rows}, {"batch_fused", &m->opt_batch_fused}, {"rows_mo", &m->opt_rows_mo}, {"debug_mo_alloc_fail", &m->opt_debug_mo_alloc_fail}, {"rows_kparts", &m->opt_rows_kparts}, {"prefill_chunk", &m->opt_prefill_chunk}, {"prefill_big_min", &m->opt_prefill_big_min}, {"prefill_mid", &m->opt_prefill_mid}, {"prefill_mid_max", &m->opt_prefill_mid_max}, {"prefill_res_mid", &m->opt_prefill_res_mid}, {"gemm_splitk", &m->opt_gemm_splitk}, {"moe_singles", &m->opt_moe_singles}, {"moe_overlap", &m->opt_moe_overlap}, {"prefill_big", &m->opt_prefill_big}, {"moe_router_fused", &m->opt_moe_router_fused}, {"tp_fuse_add", &m->opt_tp_fuse_add}, {"attn_q8", &m->opt_attn_q8}, {"attn_kt", &m->opt_attn_kt}, {"fuse_attn", &m->opt_fuse_attn}, {"fuse_ffn", &m->opt_fuse_ffn}, {"attn_post_as_residual", &m->opt_attn_post_as_residual}, {"chain_late_w2", &m->opt_chain_late_w2}, {"exact_order", &m->opt_exact_order}, {"perf_stat", &m->opt_perf_stat}, {"attn_nsplits", &m->opt_attn_nsplits}, {"attn_unload", &m->opt_attn_unload}, {"q3h_native", &m->opt_q3h_native}, {"fuse_attn_timeout_us", &m->opt_fuse_attn_timeout_us}, {"step_tail", &m->opt_step_tail}, {"graph_steps", &m->opt_graph_steps}, {"moe_device", &m->opt_moe_device}, 
        
        {"debug_layers", &m->opt_debug_layers}, {"debug_layer0", &m->opt_debug_layer0}, {"debug_hidden_in", &m->opt_debug_hidden_in}};
    for (auto &o : opts)
        if (strcmp(o.n, name) == 0) {
            *o.p = value;
            drop_graphs(m);
            return IFA_OK;
        }
    return ifa_fail(IFA_ERR_ARG, "ifa_model_set_option: unknown option '%s'", name);
}

// ids the greedy selection never offers (GetSortedTopK skips the vocabulary's unk id and Invalid-type tokens,
// src/transformer/sampling_strategy.cc:281-297): kept in the device state next to token / position so that the
// captured step needs no re-capture when they change
// (layer + 1) * 10000 + phase -> milliseconds accumulated since the last clear (ascending keys); see opt_perf_stat
int ifa_model_perf_stat(ifa_model *m, int *keys_out, float *ms_out, int cap, int *n_out, int clear)
{
    IFA_REQUIRE(m && n_out && cap >= 0 && (cap == 0 || (keys_out && ms_out)), "ifa_model_perf_stat: null pointer");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    int rc = perf_collect(m);
    if (rc) return rc;
    int n = 0;
    for (auto &kv : m->perf_map) {
        if (n < cap) { keys_out[n] = kv.first; ms_out[n] = kv.second; }
        n++;
    }
    *n_out = n;                      // (the number of keys there are: a caller with a small buffer asks again)
    if (clear) m->perf_map.clear();
    return IFA_OK;
}

int ifa_model_set_excluded_tokens(ifa_model *m, const int *ids_host, int n)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_set_excluded_tokens: model not finalized");
    IFA_REQUIRE(n >= 0 && n <= 3 && (n == 0 || ids_host), "ifa_model_set_excluded_tokens: n %d (0..3)", n);
    int v[4] = {n, -1, -1, -1};
    for (int i = 0; i < n; i++) v[1 + i] = ids_host[i];
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    IFA_HIP_CHECK(hipMemcpy(m->state + 3, v, sizeof(v), hipMemcpyHostToDevice));
    return IFA_OK;
}

int ifa_model_fused_supported(ifa_model *m, char *why, size_t why_len)
{
    IFA_REQUIRE(m, "ifa_model_fused_supported: null model");
    std::string w;
    bool ok = fused_supported(m, &w);
    if (why && why_len) { strncpy(why, w.c_str(), why_len - 1); why[why_len - 1] = 0; }
    return ok ? 1 : 0;
}

// the decode route plan (ifa_decode_route.h) for tests: the pure function, and what the model's last decode call planned
int ifa_decode_route_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == DEC_ROUTE_N_FACTS && n_out >= DEC_ROUTE_N_OUT, "ifa_decode_route_plan: %d facts, %d outputs expected", DEC_ROUTE_N_FACTS, DEC_ROUTE_N_OUT);
    DecRouteFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.head_dim >= 8 && f.max_ctx >= 1, "ifa_decode_route_plan: head_dim %d, max_ctx %d", f.head_dim, f.max_ctx);
    const DecRoute r = plan_decode_route(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_model_decode_route(ifa_model *m, int *out, int n_out)
{
    IFA_REQUIRE(m && out && n_out >= DEC_ROUTE_N_OUT + 3, "ifa_model_decode_route: %d outputs expected", DEC_ROUTE_N_OUT + 3);
    memcpy(out, &m->route, sizeof(m->route));
    out[DEC_ROUTE_N_OUT] = num_cus(); out[DEC_ROUTE_N_OUT + 1] = visible_cus(); out[DEC_ROUTE_N_OUT + 2] = waits_enabled() ? 1 : 0;
    return IFA_OK;
}

// the prompt and batched-step route plans (ifa_prompt_route.h) for tests: the pure functions, and what the model's last prompt call ran
int ifa_prompt_route_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == PROMPT_ROUTE_N_FACTS && n_out >= PROMPT_ROUTE_N_OUT, "ifa_prompt_route_plan: %d facts, %d outputs expected", PROMPT_ROUTE_N_FACTS, PROMPT_ROUTE_N_OUT);
    PromptRouteFacts f;
    memcpy(&f, facts, sizeof(f));
    const PromptRoute r = plan_prompt_route(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_batch_route_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == BATCH_ROUTE_N_FACTS && n_out >= BATCH_ROUTE_N_OUT, "ifa_batch_route_plan: %d facts, %d outputs expected", BATCH_ROUTE_N_FACTS, BATCH_ROUTE_N_OUT);
    BatchRouteFacts f;
    memcpy(&f, facts, sizeof(f));
    const BatchRoute r = plan_batch_route(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_model_prompt_route(ifa_model *m, int *out, int n_out)
{
    IFA_REQUIRE(m && out && n_out >= PROMPT_ROUTE_N_OUT, "ifa_model_prompt_route: %d outputs expected", PROMPT_ROUTE_N_OUT);
    memcpy(out, &m->prompt_route, sizeof(m->prompt_route));
    return IFA_OK;
}

// the plan an MoE layer would follow over T rows now (ifa_moe_plan.h; the facts are the engine's own: moe_plan, ifa_engine_moe.hip)
int ifa_model_moe_plan(ifa_model *m, int layer, int T, int caller_norm, int *out, int n_out)
{
    IFA_REQUIRE(m && out && n_out >= MOE_N_OUT, "ifa_model_moe_plan: %d outputs expected", MOE_N_OUT);
    IFA_REQUIRE(layer >= 0 && layer < m->cfg.layers && T >= 1, "ifa_model_moe_plan: layer %d, %d rows", layer, T);
    const Layer &L = m->layers[(size_t)layer];
    IFA_REQUIRE(m->cfg.experts > 0 && L.t[T_MOE_GATE].present(), "ifa_model_moe_plan: layer %d has no experts", layer);
    const MoePlan r = moe_plan(m, L, T, caller_norm != 0);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_model_get_buffer(ifa_model *m, const char *name, int layer, void **dptr, size_t *bytes)
{
    IFA_REQUIRE(m && name && dptr, "ifa_model_get_buffer: null pointer");
    const ifa_model_config &c = m->cfg;
    size_t b = 0; void *p = nullptr;
    if (!strcmp(name, "logits")) { p = m->logits; b = (size_t)c.vocab * 2; }
    else if (!strcmp(name, "logits_adj")) { p = m->la_adj; b = m->la_adj ? m->la_adj.cap() / m->g[T_LM_HEAD].rows * (size_t)c.vocab * 2 : 0; }
    else if (!strcmp(name, "logit_state")) { p = m->la_state; b = m->la_slots * m->g[T_LM_HEAD].rows * sizeof(unsigned); }      // [slots][vocab] u32 (null before the first reset)
    else if (!strcmp(name, "tp_logits")) { p = m->tp_logits; b = m->tp_logits ? m->g[T_LM_HEAD].rows * 2 : 0; }
    else if (!strcmp(name, "trace")) { p = m->trace; b = m->trace ? sizeof(long long) * 2048 * 8 : 0; }
    else if (!strcmp(name, "hidden")) { p = m->xn; b = (size_t)c.dim * 2; }
    else if (!strcmp(name, "x")) { p = m->x; b = (size_t)c.dim * 2; }
    else if (!strcmp(name, "x2")) { p = m->x2; b = (size_t)c.dim * 2; }
    else if (!strcmp(name, "dqkv")) { p = m->dqkv; b = ((size_t)c.heads + 2 * (size_t)c.kv_heads) * c.head_dim * 2; }
    else if (!strcmp(name, "att")) { p = m->att; b = (size_t)c.heads * c.head_dim * 2; }
    else if (!strcmp(name, "attq")) { p = m->attq; b = m->attq ? xq_image_bytes(c.heads * c.head_dim) : 0; }
    else if (!strcmp(name, "a")) { p = m->a; b = (size_t)c.dim * 2; }
    else if (!strcmp(name, "t1")) { p = m->t1; b = (size_t)c.ffn * 2; }
    else if (!strncmp(name, "rows_", 5)) {      // every row of a step's activation buffers (scratch_tokens rows; bqkv: 32)
        const size_t R = (size_t)std::max(0, m->scratch_tokens), QD = (size_t)c.heads * c.head_dim, KVD = (size_t)c.kv_heads * c.head_dim;
        const char *n = name + 5;
        if (!strcmp(n, "x")) { p = m->x; b = R * c.dim * 2; }
        else if (!strcmp(n, "xn")) { p = m->xn; b = R * c.dim * 2; }
        else if (!strcmp(n, "hn")) { p = m->hn; b = R * c.dim * 2; }
        else if (!strcmp(n, "att")) { p = m->att; b = R * QD * 2; }
        else if (!strcmp(n, "a")) { p = m->a; b = R * c.dim * 2; }
        else if (!strcmp(n, "f")) { p = m->f; b = R * c.dim * 2; }
        else if (!strcmp(n, "t1")) { p = m->t1; b = R * c.ffn * 2; }
        else if (!strcmp(n, "q")) { p = m->q; b = R * QD * 2; }
        else if (!strcmp(n, "k")) { p = m->k; b = R * KVD * 2; }
        else if (!strcmp(n, "v")) { p = m->v; b = R * KVD * 2; }
        else if (!strcmp(n, "bqkv")) { p = m->bqkv; b = m->bqkv ? (size_t)32 * (QD + 2 * KVD) * 2 : 0; }
        else return ifa_fail(IFA_ERR_ARG, "ifa_model_get_buffer: unknown buffer '%s'", name);
    }
    else if (!strncmp(name, "moe_", 4)) {       // the device-routed MoE layer's buffers, sized by the scratch capacity (scratch_tokens rows x top_k entries)
        IFA_REQUIRE(c.experts > 0, "ifa_model_get_buffer: '%s' of a model without experts", name);
        const size_t R = (size_t)std::max(0, m->scratch_tokens), cap = R * (size_t)std::max(1, c.moe_top_k), E = (size_t)c.experts, F = c.ffn;
        const char *n = name + 4;
        if (!strcmp(n, "gate")) { p = m->moe_gate; b = R * E * 2; }
        else if (!strcmp(n, "sel")) { p = m->moe_sel; b = cap * sizeof(int); }
        else if (!strcmp(n, "selw")) { p = m->moe_selw; b = cap * 2; }
        else if (!strcmp(n, "idx")) { p = m->moe_idx; b = cap * sizeof(int); }
        else if (!strcmp(n, "wdev")) { p = m->moe_wdev; b = cap * 2; }
        else if (!strcmp(n, "epos")) { p = m->moe_epos; b = cap * sizeof(int); }
        else if (!strcmp(n, "counts")) { p = m->moe_counts; b = R ? 16 * sizeof(int) : 0; }
        else if (!strcmp(n, "tiles")) { p = m->moe_tiles; b = R ? (cap / 64 + E + 1) * sizeof(MoeTile) : 0; }
        else if (!strcmp(n, "singles")) { p = m->moe_singles; b = R ? (E + 1) * sizeof(MoeSingle) : 0; }
        else if (!strcmp(n, "smalls")) { p = m->moe_smalls; b = R ? (E + 1) * sizeof(MoeTile) : 0; }
        else if (!strcmp(n, "gin")) { p = m->moe_gin; b = cap * c.dim * 2; }
        else if (!strcmp(n, "g1")) { p = m->moe_g1; b = cap * F * 2; }
        else if (!strcmp(n, "g3")) { p = m->moe_g3; b = cap * F * 2; }
        else if (!strcmp(n, "gout")) { p = m->moe_gout; b = cap * c.dim * 2; }
        else return ifa_fail(IFA_ERR_ARG, "ifa_model_get_buffer: unknown buffer '%s'", name);
    }
    else if (!strcmp(name, "kcache") || !strcmp(name, "vcache")) {
        IFA_REQUIRE(layer >= 0 && layer < c.layers && m->finalized, "ifa_model_get_buffer: layer %d", layer);
        p = name[0] == 'k' ? m->layers[(size_t)layer].kcache : m->layers[(size_t)layer].vcache;
        b = m->kv_row_bytes * (size_t)c.max_ctx;
    } else return ifa_fail(IFA_ERR_ARG, "ifa_model_get_buffer: unknown buffer '%s'", name);
    *dptr = p;
    if (bytes) *bytes = b;
    return IFA_OK;
}

void *ifa_model_stream(ifa_model *m) { return m ? (void *)m->stream : nullptr; }

int ifa_model_set_stream(ifa_model *m, ifa_stream stream)
{
    IFA_REQUIRE(m, "ifa_model_set_stream: null model");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    if (m->stream) IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->stream) (void)ifa_gemm_release_stream((ifa_stream)m->stream);
    if (m->stream && m->own_stream) IFA_HIP_CHECK(hipStreamDestroy(m->stream));
    m->stream = ifa_s(stream);
    m->own_stream = false;
    drop_graphs(m);
    return IFA_OK;
}

int ifa_model_get_tensor(ifa_model *m, int layer, int tensor_id, int *dtype, void **dptr, size_t *rows, size_t *cols)
{
    IFA_REQUIRE(m && tensor_id >= 0 && tensor_id < T_MAX, "ifa_model_get_tensor: bad arguments");
    const Tensor *t;
    if (tensor_id < 10) t = &m->g[tensor_id];
    else {
        IFA_REQUIRE(layer >= 0 && layer < m->cfg.layers, "ifa_model_get_tensor: layer %d", layer);
        t = &m->layers[(size_t)layer].t[tensor_id];
    }
    if (dtype) *dtype = t->dtype;
    if (dptr) *dptr = t->data;
    if (rows) *rows = t->rows;
    if (cols) *cols = t->cols;
    return t->present() ? IFA_OK : 1;   /* 1 = tensor not set (not an error) */
}

// W1 / W2 / W3 of one expert of a mixture-of-experts layer (the layer's own tensor ids name the dense FFN)
int ifa_model_get_expert_tensor(ifa_model *m, int layer, int expert, int tensor_id, int *dtype, void **dptr, size_t *rows, size_t *cols)
{
    IFA_REQUIRE(m && layer >= 0 && layer < m->cfg.layers, "ifa_model_get_expert_tensor: layer %d", layer);
    IFA_REQUIRE(tensor_id == T_W1 || tensor_id == T_W2 || tensor_id == T_W3, "ifa_model_get_expert_tensor: tensor id %d (w1 / w2 / w3 only)", tensor_id);
    const Layer &L = m->layers[(size_t)layer];
    IFA_REQUIRE(expert >= 0 && (size_t)expert * 3 + 2 < L.experts.size(), "ifa_model_get_expert_tensor: expert %d of layer %d", expert, layer);
    const Tensor &t = L.experts[(size_t)expert * 3 + (tensor_id == T_W1 ? 0 : (tensor_id == T_W2 ? 1 : 2))];
    if (dtype) *dtype = t.dtype;
    if (dptr) *dptr = t.data;
    if (rows) *rows = t.rows;
    if (cols) *cols = t.cols;
    return t.present() ? IFA_OK : 1;
}

} // extern "C"
