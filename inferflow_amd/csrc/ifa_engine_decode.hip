// ifa_engine_decode.hip -- the fused batch-1 decode step (GpuInferenceWorker::ProcessGpuLayer at T = 1, inference_worker.cc:762-981):
// the parameters of every fused launch, the step as a captured graph, ifa_model_decode and the per-kernel timing entry point.
#include "ifa_engine_state.h"

namespace ifae {

// Which attention launch a step takes, with which kernel instance, is planned once per decode call by plan_decode_route
// (ifa_decode_route.h; rules R1 - R10 and the measurements behind their numbers: DESIGN.md, "Decode route plan") from the facts
// decode_route_ready collects; the launches below read m->route and decide nothing.

// ------------------------------------------------------------------ dispatch
// reads one dword every `stride` bytes: warms the TLB / pulls lines towards L2+MALL
__global__ void __launch_bounds__(256) k_touch(const uint8_t *__restrict__ p, size_t bytes, size_t stride, int *sink)
{
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * stride;
    int acc = 0;
    for (; i < bytes; i += (size_t)gridDim.x * blockDim.x * stride) acc += *reinterpret_cast<const int *>(p + i);
    if (acc == 0x7FFFFFFF) *sink = acc;
}

static long long *g_trace_ptr = nullptr;   // set by ifa_model_time_kernel when the "trace" option is on

bool fused_ok(const Tensor &t, bool long_rows)
{
    if (!t.present()) return false;
    if (fused_int8(t.dtype)) return t.tiled && (long_rows ? dec_gemv_supported_long(t.dtype, t.cols) : dec_gemv_supported(t.dtype, t.cols));
    return dec_gemv_h_supported(t.dtype, t.cols) && (long_rows || t.cols <= 8192);
}

template <int EPI, int NORM>
static int launch_dec_gemv(int w_dtype, const DecGemvParams &P, int wgs_per_cu_opt, hipStream_t s)
{
    if (!fused_int8(w_dtype) && w_dtype != Q3H_NATIVE) {
        if constexpr (NORM == 2 || epi_is_moe(EPI)) return ifa_fail(IFA_ERR_STATE, "fused GEMV: dtype %d has no kernel for this launch", w_dtype);
        else return dec_gemv_h_launch(w_dtype, EPI, NORM, P, s);
    }
    return dec_gemv_launch(w_dtype, EPI, NORM, P, wgs_per_cu_opt, s, g_trace_ptr);
}

int lmhead_grid(const DecLmHeadParams &P, int wgs_per_cu_opt)
{
    const int nj = (P.cols / 8 + 63) / 64;
    const int R = nj <= 4 ? 2 : 1;
    const int nbatch = (P.rows + R - 1) / R;
    const int per_cu = wgs_per_cu_opt > 0 ? wgs_per_cu_opt : 2;
    return std::max(1, std::min(num_cus() * per_cu, (nbatch + DEC_WAVES - 1) / DEC_WAVES));
}

// the instance of nj column chunks per lane (1 .. 16; two rows per batch up to 4), with or without the norm, alone or as the step's tail
template <int NJ>
static void lmhead_go(int nj, int norm, dim3 grid, size_t smem, hipStream_t s, const DecLmHeadParams &P, const DecStepTail *Z)
{
    if constexpr (NJ <= 16) {
        constexpr int R = NJ <= 4 ? 2 : 1;
        if (nj != NJ) return lmhead_go<NJ + 1>(nj, norm, grid, smem, s, P, Z);
        if (Z) { if (norm) k_dec_lmhead_tail<NJ, R, 1><<<grid, dim3(DEC_THREADS), smem, s>>>(P, *Z); else k_dec_lmhead_tail<NJ, R, 0><<<grid, dim3(DEC_THREADS), smem, s>>>(P, *Z); }
        else if (norm) k_dec_lmhead_f16<NJ, R, 1><<<grid, dim3(DEC_THREADS), smem, s>>>(P);
        else k_dec_lmhead_f16<NJ, R, 0><<<grid, dim3(DEC_THREADS), smem, s>>>(P);
    }
}

int launch_lmhead(const DecLmHeadParams &P, int norm, int wgs_per_cu_opt, hipStream_t s, const DecStepTail *Z)
{
    const int nj = (P.cols / 8 + 63) / 64;
    if (P.cols % 8 != 0 || nj < 1 || nj > 16) return ifa_fail(IFA_ERR_ARG, "fused lm_head supports cols %% 8 == 0 and <= 8192 (got %d)", P.cols);
    dim3 grid((unsigned)lmhead_grid(P, wgs_per_cu_opt));
    const size_t smem = (((size_t)P.cols * 2 + 15) & ~(size_t)15) + 132 * 4 + 16;
    lmhead_go<1>(nj, norm, grid, smem, s, P, Z);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// self_attn.post_norm / feed_forward.post_norm (OPT / BERT-style specs): the op-by-op layer only (layer_tail_ops)
bool has_post_norms(const ifa_model *m)
{
    for (const Layer &L : m->layers) if (L.t[T_ATTN_POST_NORM].present() || L.t[T_FFN_POST_NORM].present()) return true;
    return false;
}

// Can the fused decode path run this model?  (otherwise decode falls back to forward())
bool fused_supported(const ifa_model *m, std::string *why)
{
    const ifa_model_config &c = m->cfg;
    auto fail = [&](const char *s) { if (why) *why = s; return false; };
    if (has_post_norms(m)) return fail("post norms (self_attn.post_norm / feed_forward.post_norm) use the op-by-op path");
    if (c.experts > 64 || (c.experts > 0 && (c.moe_top_k < 1 || c.moe_top_k > 8))) return fail("MoE: experts / top_k out of range");
    if ((scale_on(c.attn_out_scale) || scale_on(c.ffn_out_scale) || scale_on(c.out_scale)) && c.tp_size > 1)
        return fail("output scales (attn_out_scale / ffn_out_scale / out_scale) on a partitioned model use the op-by-op path");
    if (c.experts > 0 && (c.norm_kind != 0 || c.parallel_attn || c.share_input)) return fail("MoE layers need the sequential RMS-norm wiring");
    if (!c.full_quant_gemv) return fail("full_quant_gemv disabled");
    if (c.head_dim != 32 && c.head_dim != 48 && c.head_dim != 64 && c.head_dim != 80 && c.head_dim != 96 && c.head_dim != 128)
        return fail("fused attention supports head_dim 32/48/64/80/96/128");
    if (c.kv_dtype == Q8_B32T2 && c.head_dim % 32 != 0) return fail("Q8 KV needs head_dim % 32 == 0");
    if (dec_attn_pv_smem(c.head_dim, c.max_ctx, DEC_ATTN_MAX_SPLITS) > IFA_LDS_LIMIT) return fail("max_context_len too large for the fused attention kernels' LDS (decode falls back to the op-by-op path)");
    if (c.dim % 32 != 0 || c.ffn % 32 != 0) return fail("dim/ffn must be multiples of 32");
    if (c.dim > 8192) return fail("fused norm prologue supports dim <= 8192");
    for (const Layer &L : m->layers) {
        const bool moe = c.experts > 0 && L.t[T_MOE_GATE].present();
        if (moe) {
            if ((int)L.experts.size() != c.experts * 3 || !L.moe_table) return fail("MoE: expert tensors missing");
            for (int e = 0; e < c.experts; e++)
                for (int k = 0; k < 3; k++) {
                    const Tensor &t = L.experts[(size_t)e * 3 + k];
                    if (!t.present() || !t.tiled || !(k == 1 ? dec_gemv_supported_long(t.dtype, t.cols) : dec_gemv_supported(t.dtype, t.cols)))
                        return fail("MoE: expert weights must be in an int8-GEMV format");
                    if (!same_fmt(t.dtype, L.experts[(size_t)(k == 1 ? 1 : 0)].dtype) || t.rows != L.experts[(size_t)k].rows) return fail("MoE: experts differ in dtype / shape");
                }
        }
        const int ids_dense[] = {T_WQ, T_WK, T_WV, T_WO, T_W1, T_W2};
        const int ids_moe[] = {T_WQ, T_WK, T_WV, T_WO};
        const int *ids = moe ? ids_moe : ids_dense;
        const int n_ids = moe ? 4 : 6;
        for (int ii = 0; ii < n_ids; ii++) {
            const int id = ids[ii];
            const Tensor &t = L.t[id];
            if (!t.present()) return fail("fused path: a layer's weight matrix is missing");
            const bool plain_input = id == T_WO || id == T_W2;      // neither normalised nor gated: long rows allowed
            if (!fused_ok(t, plain_input)) return fail("fused GEMV: columns out of range for this weight format (or cols % 8 != 0 for fp16 activations)");
        }
        if (L.t[T_W3].present() && (!fused_ok(L.t[T_W3], false) || !same_fmt(L.t[T_W3].dtype, L.t[T_W1].dtype))) return fail("w1/w3 dtype mismatch");
        if (!L.t[T_ATTN_NORM].present()) return fail("pre-norm weights required");
        if (!L.t[T_FFN_NORM].present() && !c.parallel_attn) return fail("ffn pre-norm weights required");
        // (wq / wk / wv of different formats -- grouped-query models under the tensor_quant_threshold rule -- get one launch each)
    }
    const Tensor &lm = m->g[T_LM_HEAD];
    // a pipeline stage (BY_LAYER partition) may hold neither embeddings nor lm_head: checked where they are used
    if (!lm.present()) { /* middle / first stage */ }
    else if (lm.dtype == F16) {
        if (lm.cols > 8192 || lm.cols % 8 != 0) return fail("fused F16 lm_head needs cols <= 8192");
    } else if (!fused_ok(lm, false) || !m->g[T_OUT_NORM].present()) {
        return fail("fused lm_head: columns out of range for its weight format (or no output norm)");
    }
    if (m->g[T_EMBD].present() && m->g[T_EMBD].dtype != F16) return fail("F16 embeddings required");
    return true;
}

// --------------------------------------------------- fused step (enqueue only)
// Std-norm models (Falcon, Bloom, OPT ...): the norm runs as the op-level kernel (same arithmetic as the op path by
// construction) into `dst`, and the GEMV that follows takes it without a norm prologue.
int sep_norm(ifa_model *m, const half_t *x, const Tensor &w, const Tensor &b, half_t *dst)
{
    return ifa_layernorm(m->cfg.norm_kind, x, 1, (size_t)m->cfg.dim, w.data, b.data, 0.0f, m->cfg.eps, dst, (ifa_stream)m->stream);
}

// Can layer l take the attention as the tail of its QKV launch?  (the one-workgroup-per-head attention, RMS-norm wiring, q / k / v
// of one int8-path format with a kernel instance, no tensor-parallel pending sum)
static bool qkv_attn_layer_ok(const ifa_model *m, int l, int *gk_out, int *rw_out)
{
    const ifa_model_config &c = m->cfg;
    const Layer &L = m->layers[(size_t)l];
    if (c.norm_kind != 0 || c.tp_size > 1) return false;
    const Tensor &wq = L.t[T_WQ], &wk = L.t[T_WK], &wv = L.t[T_WV];
    if (!wq.present() || !wk.present() || !wv.present() || !wq.tiled || !wk.tiled || !wv.tiled) return false;
    if (!fused_int8(wq.dtype) || !same_fmt(wq.dtype, wk.dtype) || !same_fmt(wq.dtype, wv.dtype)) return false;
    if ((int)wq.rows != c.heads * c.head_dim || (int)wk.rows != c.kv_heads * c.head_dim || (int)wv.rows != c.kv_heads * c.head_dim) return false;
    return dec_qkv_attn_supported(wq.dtype, (int)wq.cols, c.heads, c.kv_heads, c.head_dim, num_cus(), gk_out, rw_out);
}

// what weights and wiring allow of the chained FFN launch (DecRouteFacts::chain_level): dense gated FFN behind an RMS pre-norm,
// sequential wiring, W1 / W3 / W2 (level 2: and Wo) of one format with an instance
static int chain_level(const ifa_model *m)
{
    const ifa_model_config &c = m->cfg;
    if (c.norm_kind != 0 || c.tp_size > 1 || c.experts != 0 || c.parallel_attn || c.share_input) return 0;
    int level = 2;
    for (int l = 0; level && l < c.layers; l++) {
        const Layer &L = m->layers[(size_t)l];
        const Tensor &wo = L.t[T_WO], &w1 = L.t[T_W1], &w3 = L.t[T_W3], &w2 = L.t[T_W2];
        if (!w1.present() || !w1.tiled || !w3.present() || !w3.tiled || !w2.present() || !w2.tiled || !L.t[T_FFN_NORM].present()
            || (int)w1.cols != c.dim || (int)w2.rows != c.dim || w2.cols != w1.rows || w3.rows != w1.rows || !same_fmt(w1.dtype, w3.dtype)
            || !dec_chain_supported(w1.dtype, w2.dtype, w1.dtype, c.dim, (int)w1.rows, false, c.dim, num_cus()))
            level = 0;
        else if (level == 2 && (!wo.present() || !wo.tiled || (int)wo.rows != c.dim
                                || !dec_chain_supported(w1.dtype, w2.dtype, wo.dtype, c.dim, (int)w1.rows, true, (int)wo.cols, num_cus())))
            level = 1;
    }
    return level;
}

static DecRouteFacts route_facts(const ifa_model *m, int reach, bool own_launches)
{
    const ifa_model_config &c = m->cfg;
    DecRouteFacts f;
    f.head_dim = c.head_dim; f.heads = c.heads; f.kv_heads = c.kv_heads; f.max_ctx = c.max_ctx; f.kv_q8 = c.kv_dtype == Q8_B32T2;
    f.reach = reach;
    f.attn_split_ctx = m->opt_attn_split_ctx; f.attn_nsplits = m->opt_attn_nsplits; f.attn_kt = m->opt_attn_kt; f.attn_unload = m->opt_attn_unload;
    f.fuse_attn = m->opt_fuse_attn; f.fuse_ffn = m->opt_fuse_ffn; f.attn_q8 = m->opt_attn_q8;
    f.waits = waits_enabled(); f.num_cus = num_cus(); f.visible_cus = visible_cus();
    f.have_attq = m->attq ? 1 : 0; f.own_launches = own_launches;
    // (the per-layer loops only where their answer can matter)
    f.tail_layers_ok = f.fuse_attn && f.waits;
    for (int l = 0; f.tail_layers_ok && l < c.layers; l++) if (!qkv_attn_layer_ok(m, l, &f.gk, &f.rw)) f.tail_layers_ok = 0;
    f.chain_level = (f.fuse_ffn && f.waits && !own_launches) ? chain_level(m) : 0;
    return f;
}

// Plans the route of a decode call that reaches `reach` keys (the captured steps hold it: they go when it changes) and allocates what
// its launches need (never under capture).  own_launches: the tensor-parallel step -- split and bucket are chosen, the fused launches are off.
int decode_route_ready(ifa_model *m, int reach, bool own_launches)
{
    const ifa_model_config &c = m->cfg;
    const DecRoute route = plan_decode_route(route_facts(m, reach, own_launches));
    m->route_reach = reach;
    if (!(route == m->route)) { m->route = route; drop_graphs(m); }
    if (route.kind == DEC_ROUTE_FUSED_TAIL && !m->qa_gran) {
        const size_t n = (size_t)c.layers * (size_t)(c.heads + 2 * c.kv_heads) * c.head_dim;
        DevBuf<unsigned long long> gran; DevBuf<unsigned> call, err;      // installed together, zeroed
        int rc;
        if ((rc = gran.alloc(n)) || (rc = call.alloc(4)) || (rc = err.alloc(4))) return rc;
        IFA_HIP_CHECK(hipMemsetAsync(gran, 0, n * 8, m->stream));
        IFA_HIP_CHECK(hipMemsetAsync(call, 0, 16, m->stream));
        IFA_HIP_CHECK(hipMemsetAsync(err, 0, 16, m->stream));
        m->qa_gran = std::move(gran); m->qa_call = std::move(call); m->qa_err = std::move(err);
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    }
    if (route.chain && !m->ch_gran) {
        const size_t n = (size_t)c.layers * (size_t)(c.dim + (int)m->layers[0].t[T_W1].rows);
        DevBuf<uint32_t> gran, flags; DevBuf<unsigned> call, err;      // installed together, zeroed
        int rc;
        if ((rc = gran.alloc(n)) || (rc = flags.alloc((size_t)c.layers * 2 * 1024))) return rc;
        IFA_HIP_CHECK(hipMemsetAsync(gran, 0, n * 4, m->stream));
        IFA_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)c.layers * 2 * 1024 * 4, m->stream));
        if (!m->qa_call) { if ((rc = call.alloc(4))) return rc; IFA_HIP_CHECK(hipMemsetAsync(call, 0, 16, m->stream)); }
        if (!m->qa_err) { if ((rc = err.alloc(4))) return rc; IFA_HIP_CHECK(hipMemsetAsync(err, 0, 16, m->stream)); }
        m->ch_gran = std::move(gran); m->ch_flags = std::move(flags);
        if (call) m->qa_call = std::move(call);
        if (err) m->qa_err = std::move(err);
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    }
    return IFA_OK;
}

// What the single GEMV launch of a role is -- the kernel format, the epilogue and the prologue -- as ONE definition for the launches
// below and for the plan the tests ask for (gemv_plan_of): the two cannot drift apart.
struct GemvRole { int dtype, epi, norm; };

// option q3h_native: the kernel format of a tensor that has its 32-byte-per-block copy (ensure_q3hn)
static int native_dtype(const ifa_model *m, const Tensor &t) { return (m->opt_q3h_native && t.q3hn && t.dtype == Q3H_B64T1) ? (int)Q3H_NATIVE : t.dtype; }

// QKV: the RMS norm in the prologue, or none behind the op-level std norm; wq's format (q / k / v of mixed formats: one launch each)
static GemvRole qkv_role(const ifa_model *m, const Layer &L) { return {L.t[T_WQ].dtype, EPI_PLAIN, m->cfg.norm_kind != 0 ? 0 : 1}; }

// Wo: norm 2 where the attention kernel left its output quantised (XqImage) and the row fits a lane's register image -- the chunked
// kernel keeps the in-kernel quantiser; no residual for a partial product and with parallel attention / a shared input (the residual
// is added once, after the FFN -- inference_worker.cc:847-851)
static GemvRole wo_role(const ifa_model *m, const Layer &L, bool partial)
{
    const ifa_model_config &c = m->cfg;
    const Tensor &wo = L.t[T_WO];
    const bool preq = m->attq && m->opt_attn_q8 && c.head_dim % 32 == 0 && (int)wo.cols == c.heads * c.head_dim && fused_int8(wo.dtype)
        && dec_gemv_supported(wo.dtype, wo.cols);
    const bool plain = partial || c.parallel_attn || c.share_input;
    return {native_dtype(m, wo), plain ? EPI_PLAIN : EPI_RESIDUAL, preq ? 2 : 0};
}

// dense W1 | W3: gated or plain activation; the FFN pre-norm in the prologue unless the model has none or it is the op-level std norm;
// both matrices of a pair in the native form, or neither
static GemvRole ffn13_role(const ifa_model *m, const Layer &L)
{
    const Tensor &w1 = L.t[T_W1], &w3 = L.t[T_W3];
    const bool glu = w3.present();
    const bool need_norm = L.t[T_FFN_NORM].present() && m->cfg.norm_kind == 0;
    const int dtw = (m->opt_q3h_native && w1.q3hn && (!glu || w3.q3hn)) ? native_dtype(m, w1) : w1.dtype;
    return {dtw, glu ? EPI_GLU : EPI_ACT, need_norm ? 1 : 0};
}

// dense W2: the in-kernel quantiser, the residual(s) unless the product is a partial one
static GemvRole w2_role(const ifa_model *m, const Layer &L, bool partial) { return {native_dtype(m, L.t[T_W2]), partial ? EPI_PLAIN : EPI_RESIDUAL, 0}; }

// the instance of a role (the combinations the roles above can name)
static int launch_role(const GemvRole &R, const DecGemvParams &P, int wgs_per_cu_opt, hipStream_t s)
{
    const int e = R.epi, n = R.norm;
    if (e == EPI_PLAIN && n == 1) return launch_dec_gemv<EPI_PLAIN, 1>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_PLAIN && n == 0) return launch_dec_gemv<EPI_PLAIN, 0>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_PLAIN && n == 2) return launch_dec_gemv<EPI_PLAIN, 2>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_RESIDUAL && n == 0) return launch_dec_gemv<EPI_RESIDUAL, 0>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_RESIDUAL && n == 2) return launch_dec_gemv<EPI_RESIDUAL, 2>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_GLU && n == 1) return launch_dec_gemv<EPI_GLU, 1>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_GLU && n == 0) return launch_dec_gemv<EPI_GLU, 0>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_ACT && n == 1) return launch_dec_gemv<EPI_ACT, 1>(R.dtype, P, wgs_per_cu_opt, s);
    if (e == EPI_ACT && n == 0) return launch_dec_gemv<EPI_ACT, 0>(R.dtype, P, wgs_per_cu_opt, s);
    return ifa_fail(IFA_ERR_STATE, "fused GEMV: no launch for epilogue %d / norm %d", e, n);
}

void qkv_params(ifa_model *m, int l, const half_t *x, DecGemvParams &P)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    memset(&P, 0, sizeof(P));
    P.x = x; P.norm_w = (const half_t *)L.t[T_ATTN_NORM].data; P.norm_b = (const half_t *)L.t[T_ATTN_NORM_B].data;
    P.multi_base = c.attn_norm_base; P.eps = c.eps; P.cols = c.dim; P.nblk = c.dim / 32;
    if (c.parallel_attn) P.xn_out = m->xn;
    const int ids[3] = {T_WQ, T_WK, T_WV}; const int bids[3] = {T_WQ_B, T_WK_B, T_WV_B};
    const size_t QDd = (size_t)c.heads * c.head_dim, KVDd = (size_t)c.kv_heads * c.head_dim;
    half_t *outs[3] = {m->dqkv, m->dqkv + QDd, m->dqkv + QDd + KVDd};
    for (int i = 0; i < 3; i++) {
        P.W0[i] = wbytes(L.t[ids[i]]); P.b0[i] = (const half_t *)L.t[bids[i]].data;
        P.y[i] = outs[i]; P.rows[i] = (int)L.t[ids[i]].rows;
    }
    P.nsets = 3;
}

// QKV GEMVs + the attention of every head in ONE launch (tag_add: distinct tags for the timing loop's repeated launches)
int launch_qkv_attn(ifa_model *m, int l, const half_t *x, unsigned tag_add)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    DecGemvParams P; qkv_params(m, l, x, P);
    DecAttnParams A; attn_params(m, l, A);
    DecQkvAttnExtra E; memset(&E, 0, sizeof(E));
    E.gran = m->qa_gran + (size_t)l * (size_t)(c.heads + 2 * c.kv_heads) * c.head_dim;
    const DecRoute &R = m->route;
    E.epoch = m->qa_call; E.epoch_add = tag_add; E.err = m->qa_err; E.timeout_us = m->opt_fuse_attn_timeout_us; E.gk = R.gk; E.unload = R.ul;
    return dec_qkv_attn_launch(L.t[T_WQ].dtype, 1, A.kv_q8 != 0, R.pb, R.kt != 0, R.ul != 0, P, A, E, c.max_ctx, m->stream);
}

int launch_qkv(ifa_model *m, int l, const half_t *x)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    DecGemvParams P; qkv_params(m, l, x, P);      // (xn_out: parallel-attention models feed the normalised input to the FFN)
    const bool std_norm = c.norm_kind != 0;
    if (std_norm) {
        int rc = sep_norm(m, x, L.t[T_ATTN_NORM], L.t[T_ATTN_NORM_B], m->xn);
        if (rc) return rc;
        P.x = m->xn; P.norm_w = nullptr; P.norm_b = nullptr; P.xn_out = nullptr;
    }
    if (m->pend.on && !std_norm) {      // x = pend.x + merged product: formed in this kernel's prologue, stored as the new layer input
        P.x = m->pend.x; P.x_add = m->pend.add; P.x_add_bias = m->pend.bias; P.xsum_out = m->pend.out;
        m->pend.on = false;
    }
    const GemvRole R = qkv_role(m, L);
    auto go = [&](int dtype, const DecGemvParams &Q) { return launch_role(GemvRole{dtype, R.epi, R.norm}, Q, m->opt_rpw_qkv, m->stream); };
    if (same_fmt(L.t[T_WQ].dtype, L.t[T_WK].dtype) && same_fmt(L.t[T_WQ].dtype, L.t[T_WV].dtype)) return go(L.t[T_WQ].dtype, P);
    // mixed formats (e.g. wq quantised, wk / wv left F16 by the threshold rule): one launch per matrix; the first one forms
    // a pending sum, the others read the stored result
    const int ids[3] = {T_WQ, T_WK, T_WV};
    for (int i = 0; i < 3; i++) {
        DecGemvParams Q = P;
        Q.nsets = 1; Q.W0[0] = P.W0[i]; Q.b0[0] = P.b0[i]; Q.y[0] = P.y[i]; Q.rows[0] = P.rows[i];
        if (i > 0) {
            Q.xn_out = nullptr;
            if (P.x_add) { Q.x = P.xsum_out; Q.x_add = nullptr; Q.x_add_bias = nullptr; Q.xsum_out = nullptr; }
        }
        int rc = go(L.t[ids[i]].dtype, Q);
        if (rc) return rc;
    }
    return IFA_OK;
}

void attn_params(ifa_model *m, int l, DecAttnParams &A)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    const int rope_dims = (int)(c.head_dim * c.partial_rotary + 0.5f);
    memset(&A, 0, sizeof(A));
    A.q = m->dqkv; A.k_new = m->dqkv + (size_t)c.heads * c.head_dim; A.v_new = A.k_new + (size_t)c.kv_heads * c.head_dim; A.kcache = (uint8_t *)L.kcache; A.vcache = (uint8_t *)L.vcache;
    A.state = m->state; A.rope_tab = m->rope_tab; A.heads = c.heads; A.kv_heads = c.kv_heads;
    A.kv_q8 = c.kv_dtype == Q8_B32T2; A.kq_scale = c.use_alibi ? 1.0f : c.kq_scale;
    A.rope_order = c.rope_order; A.rope_cols = rope_dims;
    A.alibi = c.use_alibi; A.alibi_base = c.tp_rank * c.heads; A.alibi_total = c.heads * std::max(1, c.tp_size);
    A.out = m->att; A.max_ctx = c.max_ctx; A.xq = (c.head_dim % 32 == 0) ? m->attq : nullptr; A.trace = g_trace_ptr;
}

// the route's attention launch(es): keys split over workgroups (scores in global memory: past the split threshold, or when a head's
// score row [max_ctx] does not fit the LDS), else one workgroup per head in the planned entry bucket
int launch_attn(ifa_model *m, int l)
{
    const ifa_model_config &c = m->cfg;
    // A caller that runs the attention as a launch of its own where the stored plan has none -- the step's route is the fused tail
    // (the timing entry), or no call has been planned yet (ifa_model_tp_attn driven layer by layer) -- takes the plan of the last
    // reach with launches of its own.  Pure host work: fine under capture.
    const bool unplanned = m->route.kind == DEC_ROUTE_FUSED_TAIL || (m->route.lds_attn | m->route.lds_pv) == 0;
    const DecRoute R = unplanned ? plan_decode_route(route_facts(m, m->route_reach, true)) : m->route;
    hipStream_t s = m->stream;
    DecAttnParams A; attn_params(m, l, A);
    if (R.kind == DEC_ROUTE_SPLIT) {
        if (R.error) return ifa_fail(IFA_ERR_ARG, "fused attention: max_context_len %d needs %d bytes of LDS per workgroup", c.max_ctx, R.lds_pv);
        DecAttnSplitWs ws = m->attn_ws; ws.nsplits = R.nsplits;
        const dim3 g2((unsigned)c.heads, (unsigned)R.nsplits);
        return attn_dispatch(c.head_dim, A.kv_q8 != 0, [&](auto hd, auto q8) {
            constexpr int HD = decltype(hd)::value; constexpr bool Q8 = decltype(q8)::value;
            int rc;
            if ((rc = launch_lds(k_dec_attn_scores<HD, Q8>, g2, dim3(256), (size_t)R.lds_scores, s, A, ws))) return rc;
            if ((rc = launch_lds(k_dec_attn_pv<HD, Q8>, g2, dim3(256), (size_t)R.lds_pv, s, A, ws))) return rc;
            return launch_lds(k_dec_attn_combine<HD>, dim3((unsigned)c.heads), dim3(HD), 0, s, ws, m->att.get(), A.xq, c.heads);
        });
    }
    return attn_dispatch(c.head_dim, A.kv_q8 != 0, [&](auto hd, auto q8) {
        constexpr int HD = decltype(hd)::value; constexpr bool Q8 = decltype(q8)::value;
        // head sizes with a power-of-two number of 16-byte pieces have the three entry buckets and, on an F16 cache, the K tile
        constexpr bool pow2 = HD == 32 || HD == 64 || HD == 128;
        auto go = [&](auto pb, auto kt) -> int {
            constexpr int PB = decltype(pb)::value; constexpr bool KT = decltype(kt)::value;
            if constexpr ((PB != 256 && !pow2) || (KT && (Q8 || !pow2)))
                return ifa_fail(IFA_ERR_ARG, "fused attention: no instance for head_dim %d, Q8 cache %d, %d-row bucket, K tile %d", HD, (int)Q8, PB, (int)KT);
            else
                return launch_lds(k_dec_attn<HD, Q8, false, PB, KT>, dim3((unsigned)c.heads), dim3(256), (size_t)R.lds_attn, s, A.q, A.kcache, A.vcache, A.heads, A.kv_heads, A);
        };
        auto by_kt = [&](auto pb) { return R.kt ? go(pb, std::true_type{}) : go(pb, std::false_type{}); };
        using std::integral_constant;
        return R.pb == 64 ? by_kt(integral_constant<int, 64>{}) : R.pb == 128 ? by_kt(integral_constant<int, 128>{}) : by_kt(integral_constant<int, 256>{});
    });
}

// Wo over the attention output.  partial: the un-merged product goes there (no bias, no residual); else a = Wo att (+ bias) with the
// layer input x as the residual operand
void wo_params(ifa_model *m, int l, const half_t *x, half_t *partial, DecGemvParams &P)
{
    Layer &L = m->layers[(size_t)l];
    memset(&P, 0, sizeof(P));
    P.x = m->att; P.cols = (int)L.t[T_WO].cols; P.nblk = P.cols / 32; P.eps = m->cfg.eps;
    P.W0[0] = wbytes(L.t[T_WO]); P.rows[0] = (int)L.t[T_WO].rows; P.nsets = 1;
    if (partial) { P.y[0] = partial; return; }
    P.b0[0] = (const half_t *)L.t[T_WO_B].data;
    P.y[0] = m->a; P.residual = x;
    if (scale_on(m->cfg.attn_out_scale)) P.pre_scale = m->cfg.attn_out_scale;      // Scale(self_att_out) fused in front of the residual add
}

int launch_wo(ifa_model *m, int l, const half_t *x, half_t *partial)
{
    Layer &L = m->layers[(size_t)l];
    DecGemvParams P; wo_params(m, l, x, partial, P);
    const GemvRole R = wo_role(m, L, partial != nullptr);
    if (R.norm == 2) P.x = reinterpret_cast<const half_t *>(m->attq.get());      // NORM == 2 kernels read the quantised image through P.x
    if (R.dtype == Q3H_NATIVE) P.W0[0] = (const uint8_t *)L.t[T_WO].q3hn;
    return launch_role(R, P, m->opt_rpw_wo, m->stream);
}

void moe_params(ifa_model *m, Layer &L, DecGemvParams &P, int slot, int tab_off)
{
    P.w_table = (const uint8_t *const *)L.moe_table;
    P.moe_sel = m->moe_route;
    P.moe_w = reinterpret_cast<const half_t *>(reinterpret_cast<const char *>(m->moe_route.get()) + 32);
    P.moe_acc = m->f;
    P.moe_slot = slot; P.moe_tab_off = tab_off;
}

// the input side of W1 | W3: a (the attention output + residual) behind the FFN pre-norm
static void ffn_in_params(ifa_model *m, Layer &L, DecGemvParams &P)
{
    const ifa_model_config &c = m->cfg;
    memset(&P, 0, sizeof(P));
    P.x = m->a; P.norm_w = (const half_t *)L.t[T_FFN_NORM].data; P.norm_b = (const half_t *)L.t[T_FFN_NORM_B].data;
    P.eps = c.eps; P.cols = c.dim; P.nblk = c.dim / 32; P.act_kind = c.act_kind; P.multi_base = c.ffn_norm_base;
}

// dense t1 = act(W1 n) [* (W3 n)]
void ffn13_params(ifa_model *m, int l, DecGemvParams &P)
{
    Layer &L = m->layers[(size_t)l];
    ffn_in_params(m, L, P);
    P.W0[0] = wbytes(L.t[T_W1]); P.b0[0] = (const half_t *)L.t[T_W1_B].data;
    P.y[0] = m->t1; P.rows[0] = (int)L.t[T_W1].rows; P.nsets = 1;
    if (L.t[T_W3].present()) { P.W1 = wbytes(L.t[T_W3]); P.b1 = (const half_t *)L.t[T_W3_B].data; }
}

// moe_slot >= 0: the FFN of the expert the router put in that slot (weights through L.moe_table)
int launch_ffn13(ifa_model *m, int l, int moe_slot, const half_t *x_layer, int moe_nslots)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    DecGemvParams P;
    if (moe_slot >= 0) {
        const Tensor &e1 = L.experts[0], &e3 = L.experts[2];
        ffn_in_params(m, L, P);
        moe_params(m, L, P, moe_slot, 0);
        P.W0[0] = (const uint8_t *)e1.tiled; P.W1 = (const uint8_t *)e3.tiled;   // (replaced by the table lookup)
        // moe_nslots router slots in one launch: set i = the expert of slot moe_slot + i, its product at t1 + i * ffn
        const int ns = std::max(1, std::min(3, moe_nslots));
        for (int i = 0; i < ns; i++) { P.y[i] = m->t1 + (size_t)i * e1.rows; P.rows[i] = (int)e1.rows; P.W0[i] = P.W0[0]; }
        P.nsets = ns;
        if (e3.present()) return launch_dec_gemv<EPI_MOE_GLU, 1>(e1.dtype, P, m->opt_rpw_ffn, m->stream);
        return launch_dec_gemv<EPI_MOE_ACT, 1>(e1.dtype, P, m->opt_rpw_ffn, m->stream);
    }
    ffn13_params(m, l, P);
    // FFN input (inference_worker.cc:853-872): the attention's normalised input (parallel attention), the layer input
    // (shared input) or the attention output + residual; then the FFN pre-norm if the model has one
    const half_t *ff_in = c.parallel_attn ? m->xn : (c.share_input ? x_layer : m->a);
    const GemvRole R = ffn13_role(m, L);
    P.x = ff_in;
    if (L.t[T_FFN_NORM].present() && c.norm_kind != 0) {
        int rc = sep_norm(m, ff_in, L.t[T_FFN_NORM], L.t[T_FFN_NORM_B], m->hn);
        if (rc) return rc;
        P.x = m->hn;
    }
    if (R.norm == 0) { P.norm_w = nullptr; P.norm_b = nullptr; }
    if (R.dtype == Q3H_NATIVE) {
        P.W0[0] = (const uint8_t *)L.t[T_W1].q3hn;
        if (L.t[T_W3].present()) P.W1 = (const uint8_t *)L.t[T_W3].q3hn;
    }
    if (R.norm == 1 && m->pend.on && P.x == m->pend.out) {     // the FFN input is the pending sum
        P.x = m->pend.x; P.x_add = m->pend.add; P.x_add_bias = m->pend.bias; P.xsum_out = m->pend.out;
        m->pend.on = false;
    }
    return launch_role(R, P, m->opt_rpw_ffn, m->stream);
}

// dense W2 over t1.  partial: the un-merged product goes there; else xnext = W2 t1 (+ bias) + a (+ residual2, the layer input of
// parallel / shared-input models)
void w2_params(ifa_model *m, int l, half_t *xnext, half_t *partial, const half_t *residual2, DecGemvParams &P)
{
    Layer &L = m->layers[(size_t)l];
    memset(&P, 0, sizeof(P));
    P.x = m->t1; P.cols = (int)L.t[T_W2].cols; P.nblk = P.cols / 32; P.eps = m->cfg.eps;
    P.W0[0] = wbytes(L.t[T_W2]); P.rows[0] = (int)L.t[T_W2].rows; P.nsets = 1;
    if (partial) { P.y[0] = partial; return; }
    P.b0[0] = (const half_t *)L.t[T_W2_B].data;
    P.y[0] = xnext; P.residual = m->a; P.residual2 = residual2;
    if (scale_on(m->cfg.ffn_out_scale)) P.pre_scale = m->cfg.ffn_out_scale;                               // Scale(ff_out)
    if (l + 1 == m->cfg.layers && scale_on(m->cfg.out_scale)) P.post_scale = m->cfg.out_scale;        // Scale(last layer's output)
}

int launch_w2(ifa_model *m, int l, half_t *xnext, half_t *partial, int moe_slot, bool moe_last,
                     const half_t *residual2, int moe_t1_slot)
{
    Layer &L = m->layers[(size_t)l];
    DecGemvParams P;
    if (moe_slot >= 0) {
        memset(&P, 0, sizeof(P));
        const Tensor &e2 = L.experts[1];
        moe_params(m, L, P, moe_slot, 2);
        P.x = m->t1 + (size_t)moe_t1_slot * e2.cols; P.cols = (int)e2.cols; P.eps = m->cfg.eps;      // (the gated product of this slot)
        P.W0[0] = (const uint8_t *)e2.tiled; P.rows[0] = (int)e2.rows; P.nsets = 1;
        if (partial) {      // tensor parallel: accumulate the weighted shard products; merged and finished by the caller
            P.y[0] = partial; P.moe_acc = partial;
            return launch_dec_gemv<EPI_MOE_ACC, 0>(e2.dtype, P, m->opt_rpw_w2, m->stream);
        }
        P.y[0] = moe_last ? xnext : m->f; P.residual = m->a; P.residual2 = residual2;
        if (moe_last && scale_on(m->cfg.ffn_out_scale)) P.pre_scale = m->cfg.ffn_out_scale;
        if (moe_last && l + 1 == m->cfg.layers && scale_on(m->cfg.out_scale)) P.post_scale = m->cfg.out_scale;
        if (moe_last) return launch_dec_gemv<EPI_MOE_LAST, 0>(e2.dtype, P, m->opt_rpw_w2, m->stream);
        return launch_dec_gemv<EPI_MOE_ACC, 0>(e2.dtype, P, m->opt_rpw_w2, m->stream);
    }
    w2_params(m, l, xnext, partial, residual2, P);
    const GemvRole R = w2_role(m, L, partial != nullptr);
    if (R.dtype == Q3H_NATIVE) P.W0[0] = (const uint8_t *)L.t[T_W2].q3hn;
    return launch_role(R, P, m->opt_rpw_w2, m->stream);
}

// [Wo ->] W1 | W3 -> W2 of layer l as ONE launch (ifa_decode_chain.h); x = the layer input (Wo's residual), xnext = the layer output
int launch_chain(ifa_model *m, int l, const half_t *x, half_t *xnext, unsigned tag_add)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    const bool wo = m->route.chain == 2;
    DecGemvParams PW, P, Q;       // the single launches' EPI_RESIDUAL / NORM 2, EPI_GLU / NORM 1 and EPI_RESIDUAL parameters
    if (wo) { wo_params(m, l, x, nullptr, PW); PW.x = reinterpret_cast<const half_t *>(m->attq.get()); }
    ffn13_params(m, l, P);
    w2_params(m, l, xnext, nullptr, nullptr, Q);
    DecChainExtra E; memset(&E, 0, sizeof(E));
    const size_t per = (size_t)c.dim + L.t[T_W1].rows;
    E.gran_a = m->ch_gran + (size_t)l * per; E.gran_h = E.gran_a + c.dim;
    E.flags_a = m->ch_flags + (size_t)l * 2048; E.flags_h = E.flags_a + 1024;
    E.state = m->state; E.epoch = m->qa_call; E.epoch_add = tag_add; E.err = m->qa_err; E.timeout_us = m->opt_fuse_attn_timeout_us;
    E.trace = g_trace_ptr; E.late_w2 = m->opt_chain_late_w2;
    return dec_chain_launch(L.t[T_W1].dtype, true, 1, wo, P, Q, wo ? &PW : nullptr, E, num_cus(), m->stream);
}

// can the step end in the one-launch tail?  (F16 lm_head behind the RMS / no final norm, the embedding table on this worker)
bool step_tail_ok(const ifa_model *m)
{
    const ifa_model_config &c = m->cfg;
    return m->opt_step_tail && m->g[T_LM_HEAD].present() && m->g[T_LM_HEAD].dtype == F16 && m->g[T_EMBD].present()
        && !(c.norm_kind != 0 && m->g[T_OUT_NORM].present()) && c.dim % 8 == 0 && c.dim <= 8192;
}

DecLmHeadParams lm_params(ifa_model *m, const half_t *x, half_t *logits_out)
{
    const ifa_model_config &c = m->cfg;
    DecLmHeadParams H; memset(&H, 0, sizeof(H));
    H.x = x; H.norm_w = (const half_t *)m->g[T_OUT_NORM].data; H.norm_b = (const half_t *)m->g[T_OUT_NORM_B].data;
    H.eps = c.eps; H.cols = c.dim; H.W = (const half_t *)m->g[T_LM_HEAD].data; H.logits = logits_out ? logits_out : m->logits;
    H.rows = (int)m->g[T_LM_HEAD].rows; H.xn_out = m->xn; H.multi_base = c.out_norm_base;
    return H;
}

// (allocates: not under capture)
int step_tail_ready(ifa_model *m)
{
    const int want = step_tail_ok(m) ? 1 : 0;
    if (want != m->st_on) { m->st_on = want; drop_graphs(m); }
    if (!want) return IFA_OK;
    const int grid = lmhead_grid(lm_params(m, m->x, nullptr), m->opt_rpw_lm);
    int rc;
    if ((size_t)grid > m->st_keys.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->st_keys.alloc((size_t)grid))) return rc;
    }
    if (!m->st_counter) {
        if ((rc = m->st_counter.alloc(4))) return rc;
        IFA_HIP_CHECK(hipMemsetAsync(m->st_counter, 0, 16, m->stream));
    }
    return IFA_OK;
}

// the last launch of a captured step: lm_head, argmax, state advance and the next step's gather (k_dec_lmhead_tail)
int launch_lm_tail(ifa_model *m, const half_t *x)
{
    const ifa_model_config &c = m->cfg;
    const DecLmHeadParams H = lm_params(m, x, nullptr);
    DecStepTail Z; memset(&Z, 0, sizeof(Z));
    Z.state = m->state; Z.ring = ifa_model::RING; Z.keys = m->st_keys; Z.counter = m->st_counter;
    Z.embd = (const half_t *)m->g[T_EMBD].data; Z.vocab = (int)m->g[T_EMBD].rows; Z.x_out = m->x;
    Z.rope_tab = c.rope_order ? m->rope_tab : nullptr; Z.head_dim = c.head_dim; Z.theta = c.rope_theta;
    Z.rope_dims = (int)(c.head_dim * c.partial_rotary + 0.5f); Z.embd_scale = c.embd_scale;
    return launch_lmhead(H, m->g[T_OUT_NORM].present() ? 1 : 0, m->opt_rpw_lm, m->stream, &Z);
}

int launch_gather(ifa_model *m)
{
    const ifa_model_config &c = m->cfg;
    // (debug_hidden_in: the layer input is what the caller stored in "x"; only the step's RoPE table is built)
    k_dec_gather<<<dim3(2), dim3(256), 0, m->stream>>>(m->opt_debug_hidden_in ? nullptr : (const half_t *)m->g[T_EMBD].data, m->state, c.dim, (int)m->g[T_EMBD].rows, m->x,
                                                       c.rope_order ? m->rope_tab : nullptr, c.head_dim, c.rope_theta,
                                                       (int)(c.head_dim * c.partial_rotary + 0.5f), c.embd_scale);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

int launch_lm(ifa_model *m, const half_t *x, half_t *logits_out)
{
    const ifa_model_config &c = m->cfg;
    const Tensor &lmt = m->g[T_LM_HEAD];
    if (lmt.dtype != F16) {      // quantised lm_head (<= 20-layer models, network_builder.cc:839-844): same fused GEMV as the layers
        DecGemvParams P; memset(&P, 0, sizeof(P));
        P.x = x; P.norm_w = (const half_t *)m->g[T_OUT_NORM].data; P.norm_b = (const half_t *)m->g[T_OUT_NORM_B].data;
        P.eps = c.eps; P.cols = c.dim; P.xn_out = m->xn; P.multi_base = c.out_norm_base;
        P.W0[0] = wbytes(lmt); P.rows[0] = (int)lmt.rows; P.nsets = 1;
        P.y[0] = logits_out ? logits_out : m->logits;
        return launch_dec_gemv<EPI_PLAIN, 1>(lmt.dtype, P, m->opt_rpw_lm, m->stream);
    }
    if (c.norm_kind != 0 && m->g[T_OUT_NORM].present()) {      // std final norm: op-level kernel, then the plain GEMV
        int rc = sep_norm(m, x, m->g[T_OUT_NORM], m->g[T_OUT_NORM_B], m->xn);
        if (rc) return rc;
        DecLmHeadParams H2; memset(&H2, 0, sizeof(H2));
        H2.x = m->xn; H2.eps = c.eps; H2.cols = c.dim; H2.W = (const half_t *)lmt.data; H2.logits = logits_out ? logits_out : m->logits;
        H2.rows = (int)lmt.rows;
        return launch_lmhead(H2, 0, m->opt_rpw_lm, m->stream);
    }
    return launch_lmhead(lm_params(m, x, logits_out), m->g[T_OUT_NORM].present() ? 1 : 0, m->opt_rpw_lm, m->stream);
}

int enqueue_fused_step(ifa_model *m, const StepTail &t)
{
    const ifa_model_config &c = m->cfg;
    hipStream_t s = m->stream;
    int rc;
    // st_on: the previous step's last launch (or ifa_model_decode, for a call's first step) has gathered this step's input; a
    // sampled step always gathers its own (its token is drawn by the step's last launch but one)
    if ((!m->st_on || t.kind == TAIL_SAMPLED) && (rc = launch_gather(m))) return rc;
    half_t *x = m->x, *xnext = m->x2;
    const int l_first = std::min(std::max(m->opt_debug_layer0, 0), c.layers - 1);
    const int n_layers = (m->opt_debug_layers > 0 && l_first + m->opt_debug_layers < c.layers) ? l_first + m->opt_debug_layers : c.layers;
    for (int l = l_first; l < n_layers; l++) {
        if (m->route.kind == DEC_ROUTE_FUSED_TAIL) {
            if ((rc = launch_qkv_attn(m, l, x))) return rc;
        } else {
            if ((rc = launch_qkv(m, l, x))) return rc;
            if ((rc = launch_attn(m, l))) return rc;
        }
        if (m->route.chain) {      // [Wo ->] W1 | W3 -> W2 as one launch
            if (m->route.chain == 1 && (rc = launch_wo(m, l, x))) return rc;
            if ((rc = launch_chain(m, l, x, xnext))) return rc;
            std::swap(x, xnext);
            continue;
        }
        if ((rc = launch_wo(m, l, x))) return rc;
        Layer &L = m->layers[(size_t)l];
        if (c.experts > 0 && L.t[T_MOE_GATE].present()) {
            if ((rc = launch_moe_router(m, l))) return rc;
            // the gated products of up to three router slots share one launch, then one W2 launch per slot (each accumulates
            // hfma(product, w, acc) in slot order)
            for (int k0 = 0; k0 < c.moe_top_k; k0 += 3) {
                const int ns = std::min(3, c.moe_top_k - k0);
                if ((rc = launch_ffn13(m, l, k0, nullptr, ns))) return rc;
                for (int k = k0; k < k0 + ns; k++)
                    if ((rc = launch_w2(m, l, xnext, nullptr, k, k + 1 == c.moe_top_k, nullptr, k - k0))) return rc;
            }
        } else {
            const bool extra = c.parallel_attn || c.share_input;
            if ((rc = launch_ffn13(m, l, -1, x))) return rc;
            if ((rc = launch_w2(m, l, xnext, nullptr, -1, false, extra ? x : nullptr))) return rc;
        }
        std::swap(x, xnext);
    }
    if (t.kind == TAIL_SAMPLED) return sampled_tail_enqueue(m, t, x);
    if (m->st_on) return launch_lm_tail(m, x);
    if ((rc = launch_lm(m, x))) return rc;
    k_dec_argmax_advance<<<dim3(1), dim3(1024), 0, s>>>(m->logits, (int)m->g[T_LM_HEAD].rows, m->state, ifa_model::RING);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// What the single GEMV launch of (layer, role) would run if the step were enqueued now (ifa_decode_gemv_plan.h), from the tensors, the
// options and num_cus, through the role helpers launch_qkv / launch_wo / launch_ffn13 / launch_w2 use.  The route is planned here under
// the options of NOW for the last call's reach: m->route is what the LAST call planned and stays until the next one.  out: the DecGemvPlan fields, then
// single (0: the step would not run this launch on its own -- the fused QKV + attention tail, the chained FFN launch, an MoE layer's
// expert launches or the op-by-op step take its place), dtype, epi, norm, cols, total_rows, num_cus, launches (3: q / k / v of mixed
// formats, one launch each -- the plan is wq's).
static int gemv_plan_of(ifa_model *m, int l, int role, int *out)
{
    const ifa_model_config &c = m->cfg;
    const Layer &L = m->layers[(size_t)l];
    const DecRoute R = plan_decode_route(route_facts(m, std::max(1, m->route_reach), false));
    const bool moe = c.experts > 0 && L.t[T_MOE_GATE].present();
    DecGemvFacts f;
    f.num_cus = num_cus();
    int single = m->opt_fused && fused_supported(m, nullptr), launches = 1;
    GemvRole G;
    if (role == 0) {
        const Tensor &wq = L.t[T_WQ], &wk = L.t[T_WK], &wv = L.t[T_WV];
        const bool same = same_fmt(wq.dtype, wk.dtype) && same_fmt(wq.dtype, wv.dtype);
        G = qkv_role(m, L);
        f.cols = c.dim; f.rpw = m->opt_rpw_qkv;
        f.total_rows = (int)(same ? wq.rows + wk.rows + wv.rows : wq.rows);
        launches = same ? 1 : 3;
        single = single && R.kind != DEC_ROUTE_FUSED_TAIL;
    } else if (role == 1) {
        G = wo_role(m, L, false);
        f.cols = (int)L.t[T_WO].cols; f.total_rows = (int)L.t[T_WO].rows; f.rpw = m->opt_rpw_wo;
        single = single && R.chain != 2;
    } else if (role == 2) {
        G = ffn13_role(m, L);
        f.cols = c.dim; f.total_rows = (int)L.t[T_W1].rows; f.rpw = m->opt_rpw_ffn;
        single = single && R.chain == 0 && !moe;
    } else {
        G = w2_role(m, L, false);
        f.cols = (int)L.t[T_W2].cols; f.total_rows = (int)L.t[T_W2].rows; f.rpw = m->opt_rpw_w2;
        single = single && R.chain == 0 && !moe;
    }
    f.dtype = G.dtype; f.epi = G.epi; f.norm = G.norm;
    const DecGemvPlan P = dec_gemv_plan(f);
    memcpy(out, &P, sizeof(P));
    int *x = out + DEC_GEMV_N_OUT;
    x[0] = single ? 1 : 0; x[1] = f.dtype; x[2] = f.epi; x[3] = f.norm; x[4] = f.cols; x[5] = f.total_rows; x[6] = f.num_cus; x[7] = launches;
    return IFA_OK;
}

} // namespace ifae

extern "C" {

// the decode GEMV launch plan (ifa_decode_gemv_plan.h) for tests: the pure function (no device is touched), and a model's launches
int ifa_decode_gemv_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == DEC_GEMV_N_FACTS && n_out >= DEC_GEMV_N_OUT, "ifa_decode_gemv_plan: %d facts, %d outputs expected", DEC_GEMV_N_FACTS, DEC_GEMV_N_OUT);
    DecGemvFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.num_cus >= 1 && f.total_rows >= 1, "ifa_decode_gemv_plan: num_cus %d, total_rows %d", f.num_cus, f.total_rows);
    const DecGemvPlan r = dec_gemv_plan(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_model_gemv_plan(ifa_model *m, int layer, int role, int *out, int n_out)
{
    IFA_REQUIRE(m && m->finalized && out && n_out >= DEC_GEMV_N_OUT + 8, "ifa_model_gemv_plan: a finalized model and %d outputs expected", DEC_GEMV_N_OUT + 8);
    IFA_REQUIRE(layer >= 0 && layer < m->cfg.layers && role >= 0 && role <= 3, "ifa_model_gemv_plan: layer %d, role %d (0 qkv, 1 wo, 2 ffn13, 3 w2)", layer, role);
    const Layer &L = m->layers[(size_t)layer];
    const bool have = role == 0 ? (L.t[T_WQ].present() && L.t[T_WK].present() && L.t[T_WV].present()) : role == 1 ? L.t[T_WO].present()
        : role == 2 ? L.t[T_W1].present() : L.t[T_W2].present();      // (a mixture-of-experts layer has qkv and wo, no dense w1 / w2)
    IFA_REQUIRE(have, "ifa_model_gemv_plan: layer %d has no dense matrix for role %d", layer, role);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    return gemv_plan_of(m, layer, role, out);
}

int ifa_model_decode(ifa_model *m, int first_token, int start_pos, int n_steps, int *out_tokens_host, float *elapsed_ms)
{
    StepTail none; TailCursor cur;
    return decode_impl(m, first_token, start_pos, n_steps, out_tokens_host, elapsed_ms, false, none, cur);
}

// Everything a decode call of n_steps from start_pos sets up before its first launch -- the attention variant of the contexts it
// reaches, the hand-off arenas, the captured step(s) -- without running a step: a caller that times its first call (bench.py with
// --warmup 0, a service's first request) keeps graph capture / instantiation out of it.  The KV cache and the activations are not
// touched (the token / position words are rewritten by every call anyway).
int ifa_model_decode_prepare(ifa_model *m, int start_pos, int n_steps)
{
    StepTail none; TailCursor cur;
    return decode_impl(m, 0, start_pos, n_steps, nullptr, nullptr, true, none, cur);
}

} // extern "C"

namespace ifae {

// a head's workgroup gave up waiting for its q | k | v rows (the error word the call copied back): the step's results are not valid
static int qa_err_check(ifa_model *m, int qerr)
{
    if (qerr == 0) return IFA_OK;
    (void)hipMemsetAsync(m->qa_err, 0, 16, m->stream);
    (void)hipStreamSynchronize(m->stream);
    // the waiting launches go off for this model (and, process-wide, for every model created later): the next call captures the
    // five-launch step, whose kernels wait for nothing
    m->opt_fuse_attn = 0; m->opt_fuse_ffn = 0;
    drop_graphs(m);
    waits_disable("the fused QKV + attention launch timed out waiting for sibling workgroups");
    return ifa_fail(IFA_ERR_STATE, "fused decode launch: a wait for another workgroup's rows timed out (code 0x%x: 0x5_ q | k | v / attention output, 0x6_ Wo output, 0x9_ chained FFN launch); "
                    "the results of this call are not valid -- repeat it: options fuse_attn / fuse_ffn are off now (five-launch step)", (unsigned)qerr);
}

// n greedy steps in a row as one captured, instantiated graph (replaces *graph)
static int capture_steps(ifa_model *m, int n, hipGraph_t *graph, hipGraphExec_t *exec)
{
    const StepTail greedy;
    return capture_graph(m, "decode step", exec, graph, [&] {
        int rc = IFA_OK;
        for (int i = 0; i < n && !rc; i++) rc = enqueue_fused_step(m, greedy);
        return rc;
    });
}

int decode_impl(ifa_model *m, int first_token, int start_pos, int n_steps, int *out_tokens_host, float *elapsed_ms, bool prepare_only,
                const StepTail &t, TailCursor &cur)
{
    const SampledCall *sc = t.kind == TAIL_SAMPLED ? t.sampled : nullptr;      // the call draws its tokens on the device
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode: model not finalized");
    IFA_REQUIRE(n_steps > 0 && n_steps <= ifa_model::RING, "ifa_model_decode: n_steps %d (max %d per call)", n_steps, ifa_model::RING);
    IFA_REQUIRE(start_pos >= 0 && start_pos + n_steps <= m->cfg.max_ctx, "ifa_model_decode: positions [%d,%d) exceed max_ctx %d",
                start_pos, start_pos + n_steps, m->cfg.max_ctx);
    IFA_REQUIRE(m->g[T_EMBD].present() && m->g[T_LM_HEAD].present(), "ifa_model_decode: embeddings / lm_head missing (pipeline stage worker)");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    std::string why;
    // host-driven steps, same semantics: order-exact (a failure is an error, never a silent change of arithmetic), or the op-by-op
    // fallback (also the path of option perf_stat: one launch per reference op to time)
    const bool exact = m->opt_exact_order != 0;
    if (exact || !m->opt_fused || m->opt_perf_stat || !fused_supported(m, &why)) {
        if (prepare_only) return IFA_OK;
        int tok = first_token;
        for (int i = 0; i < n_steps; i++) {
            int nt = 0;
            int rc = exact ? forward_exact(m, tok, start_pos + i, nullptr, &nt, t, cur) : forward_ops(m, &tok, 1, start_pos + i, nullptr, &nt, t, cur);
            if (rc) return rc;
            if (out_tokens_host) out_tokens_host[i] = nt;
            tok = nt;
        }
        if (elapsed_ms) *elapsed_ms = -1.0f;
        return IFA_OK;
    }
    static const bool trace_host = getenv("IFA_TRACE_DECODE") != nullptr;       // tuning aid: host-side timeline of the call on stderr
    const auto th0 = std::chrono::steady_clock::now();
    auto th = [&](const char *what) {
        if (trace_host) fprintf(stderr, "decode-host %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - th0).count());
    };
    int rc = ensure_scratch(m, 1);
    if (rc) return rc;
    if (m->opt_q3h_native && (rc = ensure_q3hn(m))) return rc;
    hipStream_t s = m->stream;
    // the attention route of this call (the captured step is re-captured when it changes)
    if ((rc = decode_route_ready(m, start_pos + n_steps))) return rc;
    const bool waits_on = m->route.kind == DEC_ROUTE_FUSED_TAIL || m->route.chain;      // launches with granule tags and an error word
    if ((rc = step_tail_ready(m))) return rc;
    m->host_pinned[0] = first_token; m->host_pinned[1] = start_pos; m->host_pinned[2] = 0;
    IFA_HIP_CHECK(hipMemcpyAsync(m->state, m->host_pinned, 3 * sizeof(int), hipMemcpyHostToDevice, s));
    if (waits_on) {      // the granule tags of this call: (call counter, position) -- consecutive steps never share one
        m->qa_calls = (m->qa_calls % 4000u) + 1u;
        m->host_pinned[6] = (int)m->qa_calls;
        IFA_HIP_CHECK(hipMemcpyAsync(m->qa_call, m->host_pinned + 6, sizeof(int), hipMemcpyHostToDevice, s));
    }
    hipGraphExec_t samp_exec = nullptr;
    if (sc) {
        if ((rc = sampled_prepare(m, t))) return rc;
        if (m->opt_graph && (rc = sampled_graph(m, t, &samp_exec))) return rc;
        if ((rc = sampled_begin(m, *sc))) return rc;
    }
    if (!sc && m->opt_graph && !m->graph_exec && (rc = capture_steps(m, 1, &m->graph, &m->graph_exec))) return rc;
    const int S = m->opt_graph_steps;
    if (!sc && m->opt_graph && S > 1 && n_steps >= S && (!m->graph_exec_n || m->graph_n_steps != S)) {
        if (m->graph_exec_n) { (void)hipGraphExecDestroy(m->graph_exec_n); m->graph_exec_n = nullptr; }
        if (m->graph_n) { (void)hipGraphDestroy(m->graph_n); m->graph_n = nullptr; }
        if ((rc = capture_steps(m, S, &m->graph_n, &m->graph_exec_n))) return rc;
        m->graph_n_steps = S;
    }
    if (prepare_only) return IFA_OK;
    th("state copies enqueued");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (elapsed_ms) { IFA_HIP_CHECK(hipEventCreate(&e0)); IFA_HIP_CHECK(hipEventCreate(&e1)); IFA_HIP_CHECK(hipEventRecord(e0, s)); }
    th("events created, first recorded");
    if (!sc && m->st_on && (rc = launch_gather(m))) return rc;      // the call's first step: its input is gathered here, every later one by the step before it
    for (int i = 0; i < n_steps;) {
        if (sc) {
            if (samp_exec) IFA_HIP_CHECK(hipGraphLaunch(samp_exec, s));
            else if ((rc = enqueue_fused_step(m, t))) return rc;
            i++;
            continue;
        }
        if (m->opt_graph && m->graph_exec_n && m->graph_n_steps == S && S > 1 && n_steps - i >= S) { IFA_HIP_CHECK(hipGraphLaunch(m->graph_exec_n, s)); i += S; continue; }
        if (m->opt_graph) IFA_HIP_CHECK(hipGraphLaunch(m->graph_exec, s));
        else if ((rc = enqueue_fused_step(m, t))) return rc;
        i++;
    }
    th("steps enqueued");
    if (elapsed_ms) IFA_HIP_CHECK(hipEventRecord(e1, s));
    if ((rc = tail_enqueue(m, t, cur, m->logits, 1))) return rc;      // (a pool: ifa_model_decode_pool only, the last step's row; the draw is inside the step)
    if (sc && (rc = sampled_copy_back(m))) return rc;
    IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned + 8, m->state + 8, sizeof(int) * (size_t)n_steps, hipMemcpyDeviceToHost, s));
    int *qerr = m->host_pinned + 8 + ifa_model::RING;
    qerr[0] = 0;
    if (waits_on) IFA_HIP_CHECK(hipMemcpyAsync(qerr, m->qa_err, 4, hipMemcpyDeviceToHost, s));
    th("copies back enqueued");
    IFA_HIP_CHECK(hipStreamSynchronize(s));
    th("stream synchronised");
    if ((rc = qa_err_check(m, qerr[0])) || (sc && (rc = sampled_finish(m, *sc)))) {
        if (elapsed_ms) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
        return rc;
    }
    if (elapsed_ms) { IFA_HIP_CHECK(hipEventElapsedTime(elapsed_ms, e0, e1)); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
    if (out_tokens_host) memcpy(out_tokens_host, m->host_pinned + 8, sizeof(int) * (size_t)n_steps);
    th("done");
    return IFA_OK;
}

} // namespace ifae

extern "C" {

int ifa_model_time_kernel(ifa_model *m, int which, int iters, float *avg_us)
{
    IFA_REQUIRE(m && m->finalized && avg_us, "ifa_model_time_kernel: bad arguments");
    IFA_REQUIRE(iters > 0 && which >= 0 && which <= 9, "ifa_model_time_kernel: which %d iters %d", which, iters);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    std::string why;
    if (!fused_supported(m, &why)) return ifa_fail(IFA_ERR_STATE, "fused path unavailable: %s", why.c_str());
    int rc = ensure_scratch(m, 1);
    if (rc) return rc;
    if (m->opt_q3h_native && (rc = ensure_q3hn(m))) return rc;
    hipStream_t s = m->stream;
    m->host_pinned[0] = 1; m->host_pinned[1] = std::min(m->cfg.max_ctx - 1, m->opt_time_pos >= 0 ? m->opt_time_pos : 64); m->host_pinned[2] = 0;
    IFA_HIP_CHECK(hipMemcpyAsync(m->state, m->host_pinned, 3 * sizeof(int), hipMemcpyHostToDevice, s));
    auto touch_layer = [&](int l) {
        const int ids[] = {T_WQ, T_WK, T_WV, T_WO, T_W1, T_W3, T_W2};
        for (int id : ids) {
            const Tensor &t = m->layers[(size_t)l].t[id];
            if (!t.tiled) continue;
            const size_t bytes = t.rows * ifa_tiled_row_bytes(t.dtype, t.cols);
            k_touch<<<dim3(8), dim3(256), 0, s>>>((const uint8_t *)t.tiled, bytes, (size_t)m->opt_touch_stride, m->state + 7);
        }
    };
    if ((rc = decode_route_ready(m, m->route_reach))) return rc;      // the last call's reach under the options of now
    if (which == 9 && !m->route.chain) return ifa_fail(IFA_ERR_STATE, "chained FFN launch unavailable for this model / option set");
    if (which == 7 && m->route.kind != DEC_ROUTE_FUSED_TAIL) return ifa_fail(IFA_ERR_STATE, "fused QKV + attention launch unavailable for this model / option set");
    auto one = [&](int i) -> int {
        if (which == 7) return launch_qkv_attn(m, i % m->cfg.layers, m->x, (unsigned)(i + 1));
        if (which == 9) return launch_chain(m, i % m->cfg.layers, m->x, m->x2, (unsigned)(i + 1));
        const int l = m->opt_bench_mode == 1 ? 0 : i % m->cfg.layers;     // rotate over layers: distinct weights every launch
        if (m->opt_bench_mode == 2) touch_layer(l);
        switch (which) {
        case 0: return launch_qkv(m, l, m->x);
        case 1: return launch_attn(m, l);
        case 2: return launch_wo(m, l, m->x);
        case 3: return launch_ffn13(m, l, -1, m->x);
        case 4: return launch_w2(m, l, m->x2);
        default: return launch_lm(m, m->x);
        }
    };
    if ((rc = launch_gather(m))) return rc;
    for (int i = 0; i < 3; i++) if ((rc = one(i))) return rc;
    if (m->opt_trace) {
        if (!m->trace && (rc = m->trace.alloc(2048 * 8))) return rc;
        IFA_HIP_CHECK(hipMemsetAsync(m->trace, 0, sizeof(long long) * 2048 * 8, s));
        g_trace_ptr = m->trace;
    }
    hipEvent_t e0, e1;
    IFA_HIP_CHECK(hipEventCreate(&e0)); IFA_HIP_CHECK(hipEventCreate(&e1));
    IFA_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) if ((rc = one(i))) return rc;
    IFA_HIP_CHECK(hipEventRecord(e1, s));
    IFA_HIP_CHECK(hipStreamSynchronize(s));
    g_trace_ptr = nullptr;
    float ms = 0;
    IFA_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = ms * 1000.0f / (float)iters;
    return IFA_OK;
}

} // extern "C"
