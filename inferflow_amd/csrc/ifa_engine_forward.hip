// ifa_engine_forward.hip -- prompts and batched steps: the op-by-op layer through the C-ABI ops the reference worker would call
// (TensorOpr / TensorMul counterparts), the four-launch prompt routes, dynamic batching.
#include "ifa_engine_state.h"

namespace ifae {

__global__ void __launch_bounds__(256) k_gather_rows(const half_t *__restrict__ embd, const int *__restrict__ tokens,
                                                     int T, int dim, int vocab, half_t *__restrict__ x, float embd_scale)
{
    const int t = blockIdx.y;
    int tok = tokens[t];
    tok = min(max(tok, 0), vocab - 1);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < dim; c += gridDim.x * blockDim.x) {
        const half_t e = embd[(size_t)tok * dim + c];
        x[(size_t)t * dim + c] = embd_scale != 0.0f ? f2h(h2f(e) * embd_scale) : e;       // LinearNorm (inference_worker.cc:447-451)
    }
}

// rows src[idx[t]] -> dst[t] (the token embedding, or an expert's rows of a batch); idx clamped to [0, n_src)
int gather_rows(ifa_model *m, const half_t *src, const int *idx_dev, int T, int dim, int n_src, half_t *dst, float scale)
{
    k_gather_rows<<<dim3(4, (unsigned)T), dim3(256), 0, m->stream>>>(src, idx_dev, T, dim, n_src, dst, scale);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// MatrixMultiplicationEx + MatrixMultiplication dispatch (inference_worker.cc:2337-2432)
int matmul(ifa_model *m, const half_t *A, int T, const Tensor &W, const Tensor &bias, half_t *C)
{
    if (!W.present()) return ifa_fail(IFA_ERR_STATE, "missing weight tensor");
    const void *b = bias.present() ? bias.data : nullptr;
    const size_t K = W.cols, N = W.rows;
    ifa_stream s = m->stream;
    const bool use_gemv = (T == 1) && (K % 32 == 0);
    if (use_gemv && W.dtype != F16 && m->cfg.full_quant_gemv && ax8_eligible(W.dtype)) {
        int rc = ifa_quantize_act_q8(A, 1, K, m->xq, s);
        if (rc) return rc;
        return ifa_gemv(W.dtype, W.data, N, K, Q8_B32T2, m->xq, b, C, s);
    }
    // a handful of rows (dynamic batching, very short prompts): weight-streaming kernel on the tiled layout
    if (T >= 2 && T <= 16 && is_q4(W.dtype) && W.tiled && m->opt_gemm_rows) {
        int rc = ifa_gemm_rows_q4(W.tiled, N, K, A, (size_t)T, b, C, s);
        if (rc != IFA_ERR_STATE) return rc;
    }
    // T > 1: MFMA GEMM with the dequantisation fused in (the reference dequantises the whole
    // tensor and calls cublasGemmEx; same arithmetic: half weights x half activations, fp32 accumulate)
    if (T > 1 && K % 8 == 0) return ifa_gemm(W.dtype, W.data, N, K, A, (size_t)T, b, C, s);
    // T == 1 with ineligible types: weights dequantised to half, fp32 accumulate per row
    for (int t = 0; t < T; t++) {
        int rc = ifa_gemv(W.dtype, W.data, N, K, F16, A + (size_t)t * K, b, C + (size_t)t * N, s);
        if (rc) return rc;
    }
    return IFA_OK;
}

int norm_rows(ifa_model *m, const half_t *x, int T, const Tensor &w, const Tensor &b, half_t *y, float base)
{
    return ifa_layernorm(m->cfg.norm_kind, x, (size_t)T, (size_t)m->cfg.dim, w.present() ? w.data : nullptr,
                         b.present() ? b.data : nullptr, base, m->cfg.eps, y, m->stream);
}

int ffn_dense(ifa_model *m, const half_t *x, int T, const Tensor &w1, const Tensor &b1, const Tensor &w3, const Tensor &b3,
                     const Tensor &w2, const Tensor &b2, half_t *out, int perf_base)
{
    int rc;
    ifa_stream s = (ifa_stream)m->stream;
    // perf_stat keys of ProcessGpuLayer_FeedForward (inference_worker.cc:1790-1880): + 730 w1, + 750 w3, + 740 activation, + 760 Mul (here ONE
    // launch, under + 760), + 780 w2 (with its input quantiser, the reference's + 770)
    const bool st = perf_base > 0;
    { PerfSpan sp(m, perf_base + 730, st); if ((rc = matmul(m, x, T, w1, b1, m->t1))) return rc; }
    if (w3.present()) {
        { PerfSpan sp(m, perf_base + 750, st); if ((rc = matmul(m, x, T, w3, b3, m->t2))) return rc; }
        PerfSpan sp(m, perf_base + 760, st);
        if ((rc = ifa_activation_mul(m->cfg.act_kind, m->t1, m->t2, (size_t)T * w1.rows, m->t1, s))) return rc;
    } else {
        PerfSpan sp(m, perf_base + 740, st);
        if ((rc = ifa_activation(m->cfg.act_kind, 0, m->t1, (size_t)T, w1.rows, m->t1, s))) return rc;
    }
    PerfSpan sp(m, perf_base + 780, st);
    return matmul(m, m->t1, T, w2, b2, out);
}

// Everything of a layer behind the attention product in m->a (bias added / shards merged): TensorOpr::Scale of the attention
// output, the residual wiring, the optional post norms, the FFN (dense or mixture of experts) and the adds in front of what
// follows -- ProcessGpuLayer, inference_worker.cc:841-965.  Shared by the prompt path and the batched step.  x: the layer
// input (on return: the layer output, m->x / m->f exchanged); attn_in: the attention's normalised input (parallel attention feeds
// it to the FFN); xn_ready: m->xn holds the next norm's output already (fused into the last Add).
//   self_attn.post_norm (:857-866): residual = a (+ x); a' = Norm(residual); the FFN reads a'; is_attn_post_as_residual picks a' as
//   the residual too.  feed_forward.post_norm (:954-965): the layer output is Norm(ffn out + residual [+ x]).
int layer_tail_ops(ifa_model *m, int l, int T, half_t *&x, const half_t *attn_in, bool &xn_ready)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    ifa_stream s = m->stream;
    const size_t D = c.dim;
    const Tensor none;
    const bool merging = tp_merging(m), seq_wiring = !c.parallel_attn && !c.share_input;
    const bool a_post = L.t[T_ATTN_POST_NORM].present(), f_post = L.t[T_FFN_POST_NORM].present();
    int rc;
    // perf_stat (layer 0 = the reference's layer_idx_for_study_): + 710 the FFN's pre-norm (with the residual Add where both are one launch),
    // + 700 ProcessGpuLayer_FeedForward as a whole (norm .. w2), + 800 what follows it (Adds, post norm; inference_worker.cc:919-950)
    const int perf_base = m->opt_perf_stat && l == 0 ? (l + 1) * 10000 : 0;
    const bool st = perf_base > 0;
    PerfSpan sp_ffn(m, perf_base + 700, st);
    PerfSpan sp_norm(m, perf_base + 710, st);
    if (scale_on(c.attn_out_scale) && (rc = ifa_scale(m->a, c.attn_out_scale, (size_t)T * D, m->a, s))) return rc;
    const half_t *ff_in = c.parallel_attn ? attn_in : (c.share_input ? x : m->a);
    const half_t *ff_n = ff_in;
    const half_t *residual = m->a;
    if (a_post) {
        if (seq_wiring && (rc = ifa_add(x, m->a, (size_t)T * D, 0, m->a, s))) return rc;
        if ((rc = norm_rows(m, m->a, T, L.t[T_ATTN_POST_NORM], L.t[T_ATTN_POST_NORM_B], m->pn, 0.0f))) return rc;
        if (m->opt_attn_post_as_residual) residual = m->pn;
        if (!c.parallel_attn && !c.share_input) ff_in = m->pn;
        ff_n = ff_in;
        if (L.t[T_FFN_NORM].present()) {
            if ((rc = norm_rows(m, ff_in, T, L.t[T_FFN_NORM], L.t[T_FFN_NORM_B], m->hn, c.ffn_norm_base))) return rc;
            ff_n = m->hn;
        }
    } else if (seq_wiring && L.t[T_FFN_NORM].present()) {          // Add(x, attn out) + ffn norm
        if ((rc = ifa_add_layernorm(c.norm_kind, x, m->a, (size_t)T, D, L.t[T_FFN_NORM].data, L.t[T_FFN_NORM_B].present() ? L.t[T_FFN_NORM_B].data : nullptr,
                                    c.ffn_norm_base, c.eps, m->a, m->hn, s))) return rc;
        ff_n = m->hn;
    } else {
        if (seq_wiring && (rc = ifa_add(x, m->a, (size_t)T * D, 0, m->a, s))) return rc;
        if (L.t[T_FFN_NORM].present()) {
            if ((rc = norm_rows(m, ff_in, T, L.t[T_FFN_NORM], L.t[T_FFN_NORM_B], m->hn, c.ffn_norm_base))) return rc;
            ff_n = m->hn;
        }
    }
    sp_norm.done();
    if (c.experts > 0 && L.t[T_MOE_GATE].present()) {
        if ((rc = moe_layer(m, L, moe_plan(m, L, T, false), ff_n, T))) return rc;
        if ((rc = tp_merge_rows(m, m->f, T, none))) return rc;          // every expert sliced like the dense FFN: one merge of the weighted sums
    } else {
        if ((rc = ffn_dense(m, ff_n, T, L.t[T_W1], L.t[T_W1_B], L.t[T_W3], L.t[T_W3_B], L.t[T_W2], merging ? none : L.t[T_W2_B], m->f, perf_base))) return rc;
        if ((rc = tp_merge_rows(m, m->f, T, L.t[T_W2_B]))) return rc;
    }
    sp_ffn.done();
    PerfSpan sp_post(m, perf_base + 800, st);
    if (scale_on(c.ffn_out_scale) && (rc = ifa_scale(m->f, c.ffn_out_scale, (size_t)T * D, m->f, s))) return rc;
    // Add(ffn out, residual) + the norm in front of what comes next: the next layer's attention norm, or the output norm
    const bool last_layer = l + 1 == c.layers;
    const Tensor &nw = last_layer ? m->g[T_OUT_NORM] : m->layers[(size_t)l + 1].t[T_ATTN_NORM];
    const Tensor &nb = last_layer ? m->g[T_OUT_NORM_B] : m->layers[(size_t)l + 1].t[T_ATTN_NORM_B];
    xn_ready = false;
    if (!a_post && !f_post && seq_wiring && nw.present() && !(last_layer && scale_on(c.out_scale))) {
        if ((rc = ifa_add_layernorm(c.norm_kind, m->f, m->a, (size_t)T, D, nw.data, nb.present() ? nb.data : nullptr,
                                    last_layer ? c.out_norm_base : c.attn_norm_base, c.eps, m->f, m->xn, s))) return rc;
        xn_ready = true;
    } else {
        if ((rc = ifa_add(m->f, residual, (size_t)T * D, 0, m->f, s))) return rc;
        if (c.parallel_attn || c.share_input)
            if ((rc = ifa_add(m->f, x, (size_t)T * D, 0, m->f, s))) return rc;
        if (f_post) {
            if ((rc = norm_rows(m, m->f, T, L.t[T_FFN_POST_NORM], L.t[T_FFN_POST_NORM_B], m->hn, 0.0f))) return rc;
            std::swap(m->f, m->hn);
        }
    }
    std::swap(m->x, m->f);
    x = m->x;
    return IFA_OK;
}

// ---- Route plans (ifa_prompt_route.h; rules P1 - P12 / B1 - B5 and the measurements behind their numbers: DESIGN.md, "Prompt route plan").
// What the plans read of the model, from ONE walk over the seven linears of every layer (minus the FFN of mixture-of-experts layers,
// which follows its own plan: ifa_moe_plan.h):
//   rows_layers  the rows GEMM (ifa_gemm_rows_mfma.hip; the five launches of the batched step, the four of a prompt of 2..32 tokens): dense or
//                device-routed layers with the sequential RMS wiring, every linear tiled Q4_B32T1 (2) or a 64-weight format with an MO copy (1)
//   big_layers   the large-tile GEMM (ifa_gemm.hip, k_gemm_big): sequential wiring, every linear a 20-byte-block Q4 tensor or a 64-weight
//                format through its Q4_B32T1A-layout copy (ensure_x32), wq / wk / wv of one format, dims in multiples of 64
//   mid_shapes   k_gemm_mid (ifa_gemm_mid.hip) reads every linear's MO copy: the shapes ensure_mo builds one for, rows in 16s
struct RouteModelFacts { int rows_layers = 0, big_layers = 0, mid_shapes = 1, has_moe = 0; };
static RouteModelFacts route_model_facts(const ifa_model *m)
{
    const ifa_model_config &c = m->cfg;
    const size_t D = c.dim, QD = (size_t)c.heads * c.head_dim, KVD = (size_t)c.kv_heads * c.head_dim, F = c.ffn;
    const bool plain = !has_post_norms(m) && !c.parallel_attn && !c.share_input && !scale_on(c.attn_out_scale) && !scale_on(c.ffn_out_scale);
    const bool hd_ok = c.head_dim == 32 || c.head_dim == 48 || c.head_dim == 64 || c.head_dim == 80 || c.head_dim == 96 || c.head_dim == 128;
    RouteModelFacts r;
    if (plain && gemm_rows_use_mfma() && c.norm_kind == 0 && !scale_on(c.out_scale) && !(D % 128 || QD % 128 || F % 128 || D > 4096 || KVD % 16) && hd_ok
        && !(c.kv_dtype == Q8_B32T2 && c.head_dim % 32 != 0) && dec_attn_smem(c.head_dim, c.max_ctx) <= IFA_LDS_LIMIT) r.rows_layers = 2;
    r.big_layers = plain && !(D % 64 || QD % 64 || F % 64);
    for (const Layer &L : m->layers) {
        const bool moe = c.experts > 0 && L.t[T_MOE_GATE].present();
        r.has_moe |= moe;
        const int ids[] = {T_WQ, T_WK, T_WV, T_WO, T_W1, T_W3, T_W2};
        for (int id : ids) {
            const Tensor &t = L.t[id];
            const bool mo_shape = t.present() && t.tiled && rows_mo_fmt(t.dtype) && t.cols % 128 == 0;      // (what ensure_mo builds a copy for)
            if (!mo_shape || t.rows % 16 != 0) r.mid_shapes = 0;
            if (moe && (id == T_W1 || id == T_W3 || id == T_W2)) continue;
            if (!t.present() || !t.tiled) r.rows_layers = 0;
            else if (!is_q4(t.dtype)) r.rows_layers = mo_shape ? std::min(r.rows_layers, 1) : 0;
            const bool b64 = (t.dtype == Q4_B64T1 || t.dtype == Q3H_B64T1) && t.tiled;
            if (!t.present() || (t.dtype != Q4_B32T1A && t.dtype != Q4_B32T1B && !b64)) r.big_layers = 0;
        }
        if (moe && !moe_plan(m, L, 2, false).device_ok) r.rows_layers = 0;      // (device_ok does not depend on the rows: M1)
        if (!L.t[T_ATTN_NORM].present() || !L.t[T_FFN_NORM].present()) r.rows_layers = r.big_layers = 0;
        if (L.t[T_ATTN_NORM_B].present() || L.t[T_FFN_NORM_B].present()) r.rows_layers = 0;
        if (L.t[T_WK].dtype != L.t[T_WQ].dtype || L.t[T_WV].dtype != L.t[T_WQ].dtype || (!moe && L.t[T_W3].dtype != L.t[T_W1].dtype)) r.big_layers = 0;
    }
    return r;
}

static PromptRouteFacts prompt_facts(const ifa_model *m, int T, bool entry)
{
    PromptRouteFacts f;
    f.T = T; f.exact_order = entry && m->opt_exact_order; f.perf_stat = m->opt_perf_stat != 0; f.prefill_chunk = entry && m->opt_prefill_chunk;
    f.prefill_mid = m->opt_prefill_mid; f.prefill_mid_max = m->opt_prefill_mid_max; f.prefill_big = m->opt_prefill_big; f.prefill_big_min = m->opt_prefill_big_min;
    f.prefill_res_mid = m->opt_prefill_res_mid; f.rows_mo = m->opt_rows_mo; f.gemm_rows = m->opt_gemm_rows; f.batch_fused = m->opt_batch_fused;
    f.gemm_splitk = m->opt_gemm_splitk; f.rows_kparts = m->opt_rows_kparts;
    f.topo = m->topo != nullptr; f.experts = m->cfg.experts;
    if (T >= 2 && !f.topo && !f.exact_order) {      // (the walk only where its answer can matter)
        const RouteModelFacts mf = route_model_facts(m);
        f.rows_layers = mf.rows_layers; f.big_layers = mf.big_layers; f.mid_shapes = mf.mid_shapes;
    }
    return f;
}

// ensure_mo for a plan that needs the copies.  A failed build switches opt_rows_mo off (it is no error of the call): what was planned with
// the copies in view -- up to 32 rows, the 64-weight formats, k_gemm_mid -- no longer holds, so the caller plans again
static int route_mo_ready(ifa_model *m, bool &replan)
{
    const int had = m->opt_rows_mo;
    const int rc = ensure_mo(m);
    replan = rc == IFA_OK && had && !m->opt_rows_mo;
    return rc;
}

// Plans a prompt of T tokens behind prefix_len (ifa_model::prompt_route) and builds the weight copies its launches read, in the plan's
// order.  entry: the call is ifa_model_forward's, whose decisions -- exact order, two passes -- are planned too; a single pass
// (forward_ops) plans without them.
int prompt_route_ready(ifa_model *m, int T, int prefix_len, bool entry, PromptRoute &R)
{
    R = plan_prompt_route(prompt_facts(m, T, entry));
    if (R.kind != PROMPT_EXACT && (T <= 0 || prefix_len < 0 || prefix_len + T > m->cfg.max_ctx))
        return ifa_fail(IFA_ERR_ARG, "forward: %d tokens at prefix %d exceed max_ctx %d", T, prefix_len, m->cfg.max_ctx);
    int rc;
    bool replan = false;
    if (R.need_mo == 1 && (rc = route_mo_ready(m, replan))) return rc;
    if (replan) R = plan_prompt_route(prompt_facts(m, T, entry));
    if (R.need_x32 && (rc = ensure_x32(m))) return rc;
    if (R.need_mo == 2 && (rc = route_mo_ready(m, replan))) return rc;
    if (replan) R = plan_prompt_route(prompt_facts(m, T, entry));
    m->prompt_route = R;
    return IFA_OK;
}

// ---- The four parameter blocks of a layer's linears on the fused routes: wq | wk | wv behind the attention norm, wo + residual, w1 / w3 + GLU
// behind the FFN norm, w2 + residual.  The prompt routes (forward_ops) and the batched step (batch_fused_layer) differ in where q | k | v
// and the layer's output go.
static const uint8_t *gm_w(const Tensor &t, int src)
{
    return (const uint8_t *)(src == GM_W_MO ? t.mo.get() : src == GM_W_X32 ? (t.x32 ? t.x32.get() : t.data.get()) : t.tiled.get());
}

static GmArgs gm_args(const ifa_model *m, int T, const GmPlan &g, const Tensor &w, const Tensor &bias, const half_t *X, size_t K, half_t *Y, size_t N)
{
    GmArgs P;
    memset(&P, 0, sizeof(P));
    P.T = T; P.eps = m->cfg.eps; P.act_kind = m->cfg.act_kind; P.mo = g.mo; P.no_waits = g.no_waits;
    P.W[0] = gm_w(w, g.src); P.rows[0] = (int)N; P.nsets = 1; P.nblk = (int)(K / 32);
    P.X = X; P.ldx = (int)K; P.bias[0] = (const half_t *)bias.data.get();
    P.Y = Y; P.ldy = (int)N;
    return P;
}

// x: the layer's input, or -- the norm being a launch of its own -- its normalised rows; qkv: one [T][q | k | v] matrix, or null for m->q, m->k, m->v
static GmArgs gm_qkv(const ifa_model *m, const Layer &L, int T, const GmPlan &g, bool norm_fused, const half_t *x, half_t *qkv)
{
    const ifa_model_config &c = m->cfg;
    const int QD = c.heads * c.head_dim, KVD = c.kv_heads * c.head_dim;
    GmArgs P = gm_args(m, T, g, L.t[T_WQ], L.t[T_WQ_B], x, c.dim, qkv, QD);
    P.W[1] = gm_w(L.t[T_WK], g.src); P.W[2] = gm_w(L.t[T_WV], g.src);
    P.rows[0] = QD; P.rows[1] = KVD; P.rows[2] = KVD; P.nsets = 3;
    if (norm_fused) { P.norm_w = (const half_t *)L.t[T_ATTN_NORM].data.get(); P.multi_base = c.attn_norm_base; }
    P.bias[1] = (const half_t *)L.t[T_WK_B].data.get(); P.bias[2] = (const half_t *)L.t[T_WV_B].data.get();
    P.ldy = qkv ? QD + 2 * KVD : 0;
    if (!qkv) { P.Yset[0] = m->q; P.Yset[1] = m->k; P.Yset[2] = m->v; P.ldyset[0] = QD; P.ldyset[1] = KVD; P.ldyset[2] = KVD; }
    return P;
}

static GmArgs gm_wo(const ifa_model *m, const Layer &L, int T, const GmPlan &g, const half_t *x)
{
    GmArgs P = gm_args(m, T, g, L.t[T_WO], L.t[T_WO_B], m->att, (size_t)m->cfg.heads * m->cfg.head_dim, m->a, m->cfg.dim);
    P.res = x; P.ldres = m->cfg.dim;
    return P;
}

static GmArgs gm_w13(const ifa_model *m, const Layer &L, int T, const GmPlan &g, bool norm_fused)
{
    GmArgs P = gm_args(m, T, g, L.t[T_W1], L.t[T_W1_B], norm_fused ? m->a : m->hn, m->cfg.dim, m->t1, m->cfg.ffn);
    P.W1 = gm_w(L.t[T_W3], g.src); P.bias1 = (const half_t *)L.t[T_W3_B].data.get();
    if (norm_fused) { P.norm_w = (const half_t *)L.t[T_FFN_NORM].data.get(); P.multi_base = m->cfg.ffn_norm_base; }
    return P;
}

static GmArgs gm_w2(const ifa_model *m, const Layer &L, int T, const GmPlan &g, half_t *out)
{
    GmArgs P = gm_args(m, T, g, L.t[T_W2], L.t[T_W2_B], m->t1, m->cfg.ffn, out, m->cfg.dim);
    P.res = m->a; P.ldres = m->cfg.dim;
    return P;
}

// A product through the kernel of its plan.  own: the plan of the route's other products -- k_gemm_mid may decline wo / w2 of a Big route
// (PromptRoute::res_mid), which the large tiles take then (with the no_waits of the plan that was tried, as ever)
static int gm_launch(ifa_model *m, const Tensor &w, GmArgs &P, const GmPlan &g, const GmPlan &own, int epi, int norm)
{
    if (g.kernel == GM_K_ROWS) return gemm_rows_mfma_launch(P, epi, norm, m->stream);
    if (g.kernel == GM_K_MID) {
        if (gemm_mid_ok(w.dtype, P, epi)) return gemm_mid(P, epi, m->stream);
        if (own.kernel == GM_K_MID) return ifa_fail(IFA_ERR_STATE, "mid-length GEMM declined a product of %zu x %zu", w.rows, w.cols);
        P.W[0] = gm_w(w, own.src); P.mo = own.mo;
    }
    return gemm_big(w.x32 ? (int)Q4_B32T1A : w.dtype, P, epi, m->stream);
}

// RoPE of q and k, and the T new K / V rows into the cache behind prefix_len (one launch where the rope kernel stores F16 rows itself)
static int rope_store_rows(ifa_model *m, Layer &L, int T, int prefix_len)
{
    const ifa_model_config &c = m->cfg;
    ifa_stream s = m->stream;
    const size_t KVD = (size_t)c.kv_heads * c.head_dim;
    int rc;
    uint8_t *kdst = (uint8_t *)L.kcache + (size_t)prefix_len * m->kv_row_bytes;
    uint8_t *vdst = (uint8_t *)L.vcache + (size_t)prefix_len * m->kv_row_bytes;
    const bool kv_f16 = c.kv_dtype != Q8_B32T2;
    bool kv_stored = false;
    if (c.rope_order != 0) {
        rc = ifa_rope_qk_store(m->q, m->k, m->v, c.head_dim, c.heads, c.kv_heads, T, prefix_len, c.rope_theta, c.rope_order, c.partial_rotary,
                               kv_f16 ? kdst : nullptr, kv_f16 ? vdst : nullptr, m->kv_row_bytes / 2, s);
        if (rc == IFA_OK) kv_stored = kv_f16;
        else if (rc != IFA_ERR_STATE) return rc;
        else {
            if ((rc = ifa_rope(m->q, c.head_dim, c.heads, T, prefix_len, c.rope_theta, c.rope_order, c.partial_rotary, s))) return rc;
            if ((rc = ifa_rope(m->k, c.head_dim, c.kv_heads, T, prefix_len, c.rope_theta, c.rope_order, c.partial_rotary, s))) return rc;
        }
    }
    if (!kv_f16) {
        if ((rc = ifa_quantize_act_q8(m->k, T, KVD, kdst, s))) return rc;
        if ((rc = ifa_quantize_act_q8(m->v, T, KVD, vdst, s))) return rc;
    } else if (!kv_stored) {
        IFA_HIP_CHECK(hipMemcpyAsync(kdst, m->k, (size_t)T * m->kv_row_bytes, hipMemcpyDeviceToDevice, m->stream));
        IFA_HIP_CHECK(hipMemcpyAsync(vdst, m->v, (size_t)T * m->kv_row_bytes, hipMemcpyDeviceToDevice, m->stream));
    }
    return IFA_OK;
}

// no_head: a chunk of a longer prompt that is not its last one -- the layers only (KV cache rows written), no lm_head / argmax / sync
// planned: the route ifa_model_forward planned for this very pass (prompt_route_ready); without it the pass plans itself
int forward_ops(ifa_model *m, const int *tokens_host, int T, int prefix_len, void *logits_out, int *next_token, const StepTail &t, TailCursor &cur,
                bool no_head, const PromptRoute *planned)
{
    const ifa_model_config &c = m->cfg;
    int rc;
    PromptRoute R;
    if (planned) R = *planned;
    else if ((rc = prompt_route_ready(m, T, prefix_len, false, R))) return rc;
    if ((rc = ensure_scratch(m, T))) return rc;
    ifa_stream s = m->stream;
    const size_t D = c.dim;
    const ifa_tp_topology *tp = m->topo;            // multi-GPU partition (ifa_model_tp_prefill): merges + stage hand-over
    const bool first_stage = !tp || tp->stage == 0, last_stage = !tp || tp->next_rank < 0 || tp->n_stages == 1;
    const bool merging = tp_merging(m);
    if (first_stage && (!m->g[T_EMBD].present() || m->g[T_EMBD].dtype != F16)) return ifa_fail(IFA_ERR_STATE, "F16 embeddings not set");
    static const bool trace_host = getenv("IFA_TRACE_FORWARD") != nullptr;
    const auto host_t0 = std::chrono::steady_clock::now();
    if (first_stage) {
        PerfSpan sp_embd(m, 1);          // (key 1: the embedding rows, InferenceEngine::Infer_Std, inference_engine.cc:1168-1176)
        IFA_HIP_CHECK(hipMemcpyAsync(m->tokens_dev, tokens_host, sizeof(int) * (size_t)T, hipMemcpyHostToDevice, m->stream));
        k_gather_rows<<<dim3(4, (unsigned)T), dim3(256), 0, m->stream>>>((const half_t *)m->g[T_EMBD].data, m->tokens_dev, T, (int)D,
                                                                          (int)m->g[T_EMBD].rows, m->x, c.embd_scale);
        IFA_LAUNCH_CHECK();
    } else if ((rc = ifa_recv(tp->world, m->x, (size_t)T * D * 2, tp->prev_rank, s))) return rc;     // the previous group's [T][dim] output
    half_t *x = m->x;
    const Tensor none;
    // small element-wise ops are one launch where the wiring allows it (each keeps its own half rounding): RoPE(q) + RoPE(k)
    // + the F16 cache rows; the residual Add + the norm that follows it (a layer is ~17 launches otherwise, and at short
    // prompts every one of them is a fixed ~5 us)
    const bool seq_wiring = !c.parallel_attn && !c.share_input;
    bool xn_ready = false;           // m->xn already holds the next norm's output (fused into the previous layer's last Add)
    // The fused routes (R: Rows, Mid, Big): the linears of a layer as FOUR launches -- (norm prologue +) wq | wk | wv into q / k / v, wo +
    // residual, (norm +) w1 / w3 + GLU, w2 + residual -- instead of seven products and four element-wise launches.  Rows: the rows GEMM
    // (ifa_gemm_rows_mfma.hip), up to 32 tokens.  Mid: k_gemm_mid on the operand-order copies, 33 .. prefill_mid_max tokens.  Big: the
    // large-tile GEMM (ifa_gemm.hip, k_gemm_big: the weights dequantised once per workgroup and step into LDS; reference-layout rows); up
    // to prefill_res_mid tokens it keeps wo and w2 (4096 output columns: 128 x 128 tiles whatever the kernel) on k_gemm_mid.
    const bool pstat = m->opt_perf_stat != 0;       // per-phase times: the op-by-op layer below (one launch per reference op), never the fused routes
    const bool fused = R.kind == PROMPT_ROWS || R.kind == PROMPT_MID || R.kind == PROMPT_BIG;
    for (int l = 0; l < c.layers && fused; l++) {
        Layer &L = m->layers[l];
        const Tensor nob;      // (the rows GEMM's route has no norm biases: rows_layers)
        const bool norm_fused = R.norm_fused != 0, rows = R.kind == PROMPT_ROWS;
        if (!norm_fused && (rc = norm_rows(m, x, T, L.t[T_ATTN_NORM], rows ? nob : L.t[T_ATTN_NORM_B], m->xn, c.attn_norm_base))) return rc;
        GmArgs P = gm_qkv(m, L, T, R.qkv, norm_fused, norm_fused ? x : m->xn, nullptr);
        if ((rc = gm_launch(m, L.t[T_WQ], P, R.qkv, R.qkv, GM_PLAIN, norm_fused))) return rc;
        if ((rc = rope_store_rows(m, L, T, prefix_len))) return rc;
        if ((rc = ifa_attention(m->q, L.kcache, L.vcache, c.kv_dtype, prefix_len + T, T, prefix_len, c.heads, c.kv_heads,
                                c.head_dim, c.use_alibi ? 1.0f : c.kq_scale, c.use_alibi, c.tp_rank * c.heads,
                                c.heads * std::max(1, c.tp_size), m->att, s))) return rc;
        P = gm_wo(m, L, T, R.wo, x);
        if ((rc = gm_launch(m, L.t[T_WO], P, R.wo, R.qkv, GM_RESIDUAL, 0))) return rc;
        if (!norm_fused && (rc = norm_rows(m, m->a, T, L.t[T_FFN_NORM], rows ? nob : L.t[T_FFN_NORM_B], m->hn, c.ffn_norm_base))) return rc;
        if (c.experts > 0 && L.t[T_MOE_GATE].present()) {      // (Big only) mixture of experts: the attention half fused, the expert FFNs device-routed
            if ((rc = moe_layer(m, L, moe_plan(m, L, T, false), m->hn, T))) return rc;
            if ((rc = ifa_add(m->f, m->a, (size_t)T * D, 0, m->f, s))) return rc;
            std::swap(m->x, m->f);
            x = m->x;
            continue;
        }
        P = gm_w13(m, L, T, R.w13, norm_fused);
        if ((rc = gm_launch(m, L.t[T_W1], P, R.w13, R.qkv, GM_GLU, norm_fused))) return rc;
        P = gm_w2(m, L, T, R.w2, m->f);
        if ((rc = gm_launch(m, L.t[T_W2], P, R.w2, R.qkv, GM_RESIDUAL, 0))) return rc;
        std::swap(m->x, m->f);
        x = m->x;
    }
    for (int l = fused ? c.layers : 0; l < c.layers; l++) {
        Layer &L = m->layers[l];
        // perf_stat spans in the reference's key space (inference_worker.cc:296-322, 806-950, 1030-1400): the whole layer under + 0 for layers
        // 0..5; for layer 0 (layer_idx_for_study_) + 300 = ProcessGpuLayer_Attention as a whole, + 10 its pre-norm, + 30 the q / k / v products
        // (with their input quantisers: the reference's + 20), + 50 RoPE + cache rows, + 60 scores / softmax / V product, + 90 wo (+ bias, merge)
        const int pbase = (l + 1) * 10000;
        const bool st = pstat && l == 0;
        PerfSpan sp_layer(m, pbase + 0, pstat && l <= 5);
        PerfSpan sp_attn(m, pbase + 300, st);
        const half_t *attn_in = x;
        if (L.t[T_ATTN_NORM].present()) {
            PerfSpan sp(m, pbase + 10, st);
            if (!xn_ready && (rc = norm_rows(m, x, T, L.t[T_ATTN_NORM], L.t[T_ATTN_NORM_B], m->xn, c.attn_norm_base))) return rc;
            attn_in = m->xn;
        }
        xn_ready = false;
        {
            PerfSpan sp(m, pbase + 30, st);
            if ((rc = matmul(m, attn_in, T, L.t[T_WQ], L.t[T_WQ_B], m->q))) return rc;
            if ((rc = matmul(m, attn_in, T, L.t[T_WK], L.t[T_WK_B], m->k))) return rc;
            if ((rc = matmul(m, attn_in, T, L.t[T_WV], L.t[T_WV_B], m->v))) return rc;
        }
        {
            PerfSpan sp(m, pbase + 50, st);
            if ((rc = rope_store_rows(m, L, T, prefix_len))) return rc;
        }
        {
            PerfSpan sp(m, pbase + 60, st);
            if ((rc = ifa_attention(m->q, L.kcache, L.vcache, c.kv_dtype, prefix_len + T, T, prefix_len, c.heads, c.kv_heads,
                                    c.head_dim, c.use_alibi ? 1.0f : c.kq_scale, c.use_alibi, c.tp_rank * c.heads,
                                    c.heads * std::max(1, c.tp_size), m->att, s))) return rc;
        }
        {
            PerfSpan sp(m, pbase + 90, st);
            if ((rc = matmul(m, m->att, T, L.t[T_WO], merging ? none : L.t[T_WO_B], m->a))) return rc;
            if ((rc = tp_merge_rows(m, m->a, T, L.t[T_WO_B]))) return rc;       // BY_TENSOR: sum of the ranks' partial products, bias after
        }
        sp_attn.done();
        if ((rc = layer_tail_ops(m, l, T, x, attn_in, xn_ready))) return rc;
    }
    if (!last_stage) {       // BY_LAYER / HYBRID: hand the [T][dim] output to the next device group, then learn the token
        if ((rc = ifa_send(tp->world, x, (size_t)T * D * 2, tp->next_rank, s))) return rc;
        if ((rc = tp_argmax_scratch(m, 1))) return rc;
        if ((rc = ifa_broadcast(tp->world, m->tp_tok, 4, tp->token_src, s))) return rc;
        IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned, m->tp_tok, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if (next_token) *next_token = m->host_pinned[0];
        return IFA_OK;
    }
    const bool all_rows = logits_out || t.kind == TAIL_SCORE;      // the lm_head over every row: for the caller's buffer, or for a scoring prompt
    if (no_head && !all_rows) return IFA_OK;
    PerfSpan sp_out(m, 1000009);         // (ProcessPostLayer: output norm + lm_head, inference_worker.cc:326-336, 673-675)
    if (scale_on(c.out_scale) && (rc = ifa_scale(x, c.out_scale, (size_t)T * D, x, s))) return rc;
    const half_t *hfin = x;
    if (m->g[T_OUT_NORM].present()) {
        if (!xn_ready && (rc = norm_rows(m, x, T, m->g[T_OUT_NORM], m->g[T_OUT_NORM_B], m->xn, c.out_norm_base))) return rc;
        hfin = m->xn;
    } else {
        IFA_HIP_CHECK(hipMemcpyAsync(m->xn, x, (size_t)T * D * 2, hipMemcpyDeviceToDevice, m->stream));
    }
    const Tensor &lm = m->g[T_LM_HEAD];
    const size_t V = lm.rows;                        // (this rank's vocabulary shard under tensor parallelism)
    int t0 = all_rows ? 0 : T - 1;
    if (all_rows) { if ((rc = matmul(m, hfin, T, lm, none, m->logits))) return rc; }
    else if (lm.dtype == F16 && D % 8 == 0 && D <= 8192) {
        // the last row only: the decode step's lm_head kernel on the normalised row (same per-row chain as the op-level GEMV --
        // bit-identical logits -- at 6 TB/s instead of 1.1: 232 -> 45 us per prompt, rocprofv3 r06)
        DecLmHeadParams H2; memset(&H2, 0, sizeof(H2));
        H2.x = hfin + (size_t)t0 * D; H2.eps = c.eps; H2.cols = (int)D; H2.W = (const half_t *)lm.data; H2.logits = m->logits + (size_t)t0 * V; H2.rows = (int)V;
        if ((rc = launch_lmhead(H2, 0, m->opt_rpw_lm, m->stream))) return rc;
    }
    else { if ((rc = matmul(m, hfin + (size_t)t0 * D, 1, lm, none, m->logits + (size_t)t0 * V))) return rc; }
    sp_out.done();
    if (logits_out) IFA_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)T * V * 2, hipMemcpyDeviceToDevice, m->stream));
    if (tp) {                // distributed argmax of the last row over the group's shards (+ announcement to the other groups)
        if ((rc = tp_pick_rows(m, *tp, m->logits + (size_t)(T - 1) * V, V, (int)V, 1))) return rc;
        if (tp->n_stages > 1 && (rc = ifa_broadcast(tp->world, m->tp_tok, 4, tp->token_src, s))) return rc;
        IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned, m->tp_tok, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    } else {
        if ((rc = ifa_argmax_masked(m->logits + (size_t)(T - 1) * V, V, m->state + 3, m->state, s))) return rc;
        IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned, m->state, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        // (all_rows: the T rows; otherwise only the last row is there, and a single-query pool reads that one)
        if ((rc = tail_enqueue(m, t, cur, all_rows ? m->logits : m->logits + (size_t)(T - 1) * V, all_rows ? T : 1))) return rc;
    }
    const auto host_t1 = std::chrono::steady_clock::now();
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (pstat && (rc = perf_collect(m))) return rc;
    if ((rc = wait_err_check("forward step"))) { drop_graphs(m); return rc; }      // (a split-K / K-parts wait gave up: the step is not valid; those launches are off now)
    if (trace_host)      // how much of a step is the host enqueuing (launch-bound) vs the GPU draining what was enqueued
        fprintf(stderr, "forward T=%d: enqueue %.3f ms, total %.3f ms\n", T, std::chrono::duration<double, std::milli>(host_t1 - host_t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count());
    if (next_token) *next_token = m->host_pinned[0];
    return IFA_OK;
}

// row r of k / v -> position rows[r].n_ctx - 1 of its query's cache (F16 copy or Q8_B32T2 quantisation, 32 lanes per block)
template <bool Q8>
__global__ void __launch_bounds__(256) k_kv_store_rows(const half_t *__restrict__ k, const half_t *__restrict__ v, int kv_dim,
                                                       size_t row_bytes, const AttnRowH *__restrict__ rows)
{
    const int r = blockIdx.x, which = blockIdx.y;
    const half_t *src = (which ? v : k) + (size_t)r * kv_dim;
    uint8_t *dst = (uint8_t *)(which ? rows[r].vc : rows[r].kc) + (size_t)(rows[r].n_ctx - 1) * row_bytes;
    if constexpr (!Q8) {
        for (int c = threadIdx.x; c < kv_dim; c += 256) reinterpret_cast<half_t *>(dst)[c] = src[c];
    } else {
        const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
        for (int b = grp; b < kv_dim / 32; b += 8) {      // Tensor_QuantizeQ8_B32T2_Alg2_Kernel (tensor_quant.h:44-82)
            const float val = h2f(src[b * 32 + lane]);
            float mx = fabsf(val);
#pragma unroll
            for (int m2 = 16; m2 > 0; m2 >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m2, 32));
            const float sc = mx / 127;
            int qv = sc <= 0.000001f ? 0 : (int)roundf(val / sc);
            qv = min(max(qv, -128), 127);
            uint8_t *blk = dst + (size_t)b * 34;
            blk[2 + lane] = (uint8_t)(int8_t)qv;
            if (lane == 0) *reinterpret_cast<uint16_t *>(blk) = __builtin_bit_cast(uint16_t, f2h(sc));
        }
    }
}

// ---- the batched step as five launches per layer (the structure of the batch-1 step: ifa_gemm_rows_mfma.hip with the norm
// prologue / GLU / residual epilogues, k_dec_attn<.., BATCH>): dense models with the sequential RMS wiring, every linear in
// tiled Q4_B32T1 or with an MO copy (rows_layers), 2..16 queries, up to 32 from the MO copies.  Everything else takes the op-by-op rows
// of forward_batch.
// batch_route_ready plans a batched step of n rows and builds what it needs before its launches (and its capture).  entry: the call is
// ifa_model_decode_batch's, whose decisions -- exact order, several steps -- are planned too, and whose steps make themselves ready.
static int batch_route_ready(ifa_model *m, int n, bool logits_out, bool entry, BatchRoute &R)
{
    BatchRouteFacts f;
    f.n = n; f.exact_order = entry && m->opt_exact_order; f.may_chunk = entry;
    f.rows_mo = m->opt_rows_mo; f.gemm_rows = m->opt_gemm_rows; f.batch_fused = m->opt_batch_fused; f.rows_kparts = m->opt_rows_kparts;
    f.batch_graph = m->opt_batch_graph; f.graph = m->opt_graph; f.topo = m->topo != nullptr; f.logits_out = logits_out;
    if (!f.exact_order) { const RouteModelFacts mf = route_model_facts(m); f.rows_layers = mf.rows_layers; f.has_moe = mf.has_moe; }
    R = plan_batch_route(f);
    if (entry) return IFA_OK;      // (its steps make themselves ready)
    int rc;
    if (R.need_mo) {
        bool replan = false;
        if ((rc = route_mo_ready(m, replan))) return rc;
        if (replan) { f.rows_mo = m->opt_rows_mo; R = plan_batch_route(f); }
        if (R.kind == BATCH_FUSED && (rc = gemm_rows_kparts_reserve(m->stream))) return rc;
    }
    // the side stream of the singles' fork (M10) exists before a capture begins (the MO tables its plan reads were built just above)
    for (const Layer &L : m->layers)
        if (f.has_moe && L.t[T_MOE_GATE].present() && moe_plan(m, L, n, R.kind == BATCH_FUSED).side_stream) return ensure_side_stream(m);
    return IFA_OK;
}

// what ifa_model_decode_batch would run for n rows now: the plan only, nothing is built (ifa_model_decode_batch_steps asks before it touches anything)
int batch_route_of_call(ifa_model *m, int n, BatchRoute &R) { return batch_route_ready(m, n, false, true, R); }

static int batch_fused_layer(ifa_model *m, const BatchRoute &R, int l, int n, const half_t *x, half_t *xnext, const void *rows_l, bool draft)
{
    const ifa_model_config &c = m->cfg;
    Layer &L = m->layers[(size_t)l];
    const size_t D = c.dim, QD = (size_t)c.heads * c.head_dim, KVD = (size_t)c.kv_heads * c.head_dim;
    int rc;
    // 1. RmsNorm -> wq | wk | wv  (one virtual row space, one [n][q | k | v] output)
    // (9..16 queries: the activation rows are staged in chunks of 2048 columns, so the norm runs as its own launch; MO layout: 16 rows x
    // 4096 columns are one chunk too; 17..32 rows: chunked)
    const bool norm_fused = R.norm_fused != 0;
    const Tensor nob;
    if (!norm_fused && (rc = norm_rows(m, x, n, L.t[T_ATTN_NORM], nob, m->xn, c.attn_norm_base))) return rc;
    GmArgs P = gm_qkv(m, L, n, R.gm, norm_fused, norm_fused ? x : m->xn, m->bqkv);
    if ((rc = gm_launch(m, L.t[T_WQ], P, R.gm, R.gm, GM_PLAIN, norm_fused))) return rc;
    // 2. RoPE, KV store, attention of every query on its own cache.  Draft step (the n rows are consecutive positions of ONE slot): the
    // K / V rows of all of them go to the cache in a launch of their own first, and the attention kernel leaves the cache alone
    if (draft && (rc = draft_kv_store_launch(m, n, m->bqkv + QD, m->bqkv + QD + KVD, (int)(QD + 2 * KVD), rows_l))) return rc;
    {
        DecAttnParams A; attn_params(m, l, A);      // the batch-1 step's; per row: q | k | v, positions and caches (rows_l), no quantised image
        A.q = m->bqkv; A.k_new = m->bqkv + QD; A.v_new = A.k_new + KVD; A.kcache = nullptr; A.vcache = nullptr;
        A.rope_tab = m->brope; A.batch_rows = rows_l; A.q_stride = (int)(QD + 2 * KVD);
        A.skip_store = draft ? 1 : 0; A.xq = nullptr; A.trace = nullptr;
        const size_t asmem = dec_attn_smem(c.head_dim, c.max_ctx);
        const dim3 grid((unsigned)c.heads, (unsigned)n), block(256);
        rc = attn_dispatch(c.head_dim, A.kv_q8 != 0, [&](auto hd, auto q8) {
            return launch_lds(k_dec_attn<decltype(hd)::value, decltype(q8)::value, true>, grid, block, asmem, m->stream,
                              A.q, nullptr, nullptr, A.heads, A.kv_heads, A);
        });
        if (rc) return rc;
    }
    // 3. wo (+ bias) + residual
    P = gm_wo(m, L, n, R.gm, x);
    if ((rc = gm_launch(m, L.t[T_WO], P, R.gm, R.gm, GM_RESIDUAL, 0))) return rc;
    if (c.experts > 0 && L.t[T_MOE_GATE].present()) {
        // mixture of experts: norm, the expert FFNs over the n rows, residual -- all three the layer's with the fused rows router (M5)
        Tensor none;
        const MoePlan MP = moe_plan(m, L, n, true);
        if (MP.router == MOE_ROUTER_FUSED) return moe_layer(m, L, MP, m->hn, n, m->a, m->a, xnext);
        if ((rc = norm_rows(m, m->a, n, L.t[T_FFN_NORM], none, m->hn, c.ffn_norm_base))) return rc;
        if ((rc = moe_layer(m, L, MP, m->hn, n))) return rc;
        return ifa_add(m->f, m->a, (size_t)n * D, 0, xnext, (ifa_stream)m->stream);
    }
    // 4. RmsNorm -> w1, w3 -> act(w1 x) * (w3 x)
    if (!norm_fused && (rc = norm_rows(m, m->a, n, L.t[T_FFN_NORM], nob, m->hn, c.ffn_norm_base))) return rc;
    P = gm_w13(m, L, n, R.gm, norm_fused);
    if ((rc = gm_launch(m, L.t[T_W1], P, R.gm, R.gm, GM_GLU, norm_fused))) return rc;
    // 5. w2 (+ bias) + residual -> the next layer's input
    P = gm_w2(m, L, n, R.gm, xnext);
    return gm_launch(m, L.t[T_W2], P, R.gm, R.gm, GM_RESIDUAL, 0);
}

int forward_batch(ifa_model *m, int n, const int *tokens_host, const int *pos_host, const int *slot_host, int *next_tokens,
                  void *logits_out, const StepTail &t, TailCursor &cur, bool draft)
{
    const bool fed = t.kind == TAIL_FED, fed_next = fed && !t.fed_first;
    const ifa_model_config &c = m->cfg;
    const int n_slots = m->slots.empty() ? 1 : (int)m->slots.size();
    int max_ctx = 0;
    for (int r = 0; r < n; r++) {
        if (pos_host[r] < 0 || pos_host[r] >= c.max_ctx) return ifa_fail(IFA_ERR_ARG, "decode_batch: position %d outside max_ctx %d", pos_host[r], c.max_ctx);
        if (slot_host[r] < 0 || slot_host[r] >= n_slots) return ifa_fail(IFA_ERR_ARG, "decode_batch: KV slot %d of %d", slot_host[r], n_slots);
        // (draft step, ifa_model_decode_draft: every row on the same slot, row r behind rows [0, r) of this very step)
        for (int r2 = 0; r2 < r && !draft; r2++) if (slot_host[r2] == slot_host[r]) return ifa_fail(IFA_ERR_ARG, "decode_batch: KV slot %d used twice", slot_host[r]);
        max_ctx = std::max(max_ctx, pos_host[r] + 1);
    }
    int rc = ensure_scratch(m, n);
    if (rc) return rc;
    ifa_stream s = m->stream;
    const int T = n;
    const size_t D = c.dim, KVD = (size_t)c.kv_heads * c.head_dim, L_ = m->layers.size();
    if (!m->g[T_EMBD].present() || m->g[T_EMBD].dtype != F16) return ifa_fail(IFA_ERR_STATE, "F16 embeddings not set");
    const ifa_tp_topology *tp = m->topo;            // tensor-parallel group (ifa_model_tp_decode_batch): merges + distributed argmax
    if (tp && tp->n_stages > 1) return ifa_fail(IFA_ERR_ARG, "decode_batch: layer groups are not batched (tensor-parallel groups only)");
    const bool merging = tp_merging(m);
    // per-step tables: positions, and for every layer the (k cache, v cache, context) of each row's query
    const size_t tab_bytes = L_ * (size_t)n * sizeof(AttnRowH) + 2 * (size_t)n * sizeof(int);
    if (tab_bytes > m->batch_tab.cap()) {
        drop_graphs(m);                            // the captured steps hold the old table addresses
        if ((rc = m->batch_tab.reserve(tab_bytes))) return rc;
    }
    AttnRowH *rows_h = (AttnRowH *)m->batch_tab.pin.get();
    int *pos_pin = (int *)(rows_h + L_ * (size_t)n);
    // (a later step of a device-fed call: the tables are the device's, and the pinned twin may still be on its way there)
    for (size_t l = 0; l < L_ && !fed_next; l++)
        for (int r = 0; r < n; r++) {
            AttnRowH &a = rows_h[l * (size_t)n + r];
            a.kc = kv_ptr(m, l, slot_host[r], false); a.vc = kv_ptr(m, l, slot_host[r], true); a.n_ctx = pos_host[r] + 1; a.pad = 0;
        }
    for (int r = 0; r < n && !fed_next; r++) { pos_pin[r] = pos_host[r]; pos_pin[n + r] = tokens_host[r]; }
    const AttnRowH *rows_d = (const AttnRowH *)m->batch_tab.dev.get();
    const int *pos_d = (const int *)(rows_d + L_ * (size_t)n);
    const int *tok_d = pos_d + n;
    // Everything the device does in a step depends on the step only through the tables above (fixed addresses), so
    // for dense models the whole step -- table upload included -- is captured once per batch size and replayed.
    // (measured on Llama-2-7B Q4: the op-by-op step is bound by the small-T GEMM kernels, ~6.7 ms with or without the graph, so its replay
    //  is opt-in: set_option("batch_graph", 1).  The fused step -- five launches per layer, MoE layers routed on the device -- is
    //  launch-bound without a graph, so it is replayed)
    BatchRoute R;
    if ((rc = batch_route_ready(m, n, logits_out != nullptr, false, R))) return rc;
    const bool fused = R.kind == BATCH_FUSED, use_graph = R.captured != 0;
    const int attn_ctx = use_graph ? c.max_ctx : max_ctx;     // LDS sizing of the attention kernel must not depend on the step
    if (fed && (!fused || !use_graph || draft)) return ifa_fail(IFA_ERR_STATE, "decode_batch_steps: the step of %d rows is not one fused, captured step", n);
    std::map<int, hipGraphExec_t> &graphs = fed ? m->fed_graphs : draft ? m->draft_graphs : m->batch_graphs;
    // device-fed call: the first step's tables go up here, once, outside the captured step
    if (fed && t.fed_first) IFA_HIP_CHECK(hipMemcpyAsync(m->batch_tab.dev, m->batch_tab.pin, tab_bytes, hipMemcpyHostToDevice, m->stream));
    auto body = [&]() -> int {
    if (!fed) IFA_HIP_CHECK(hipMemcpyAsync(m->batch_tab.dev, m->batch_tab.pin, tab_bytes, hipMemcpyHostToDevice, m->stream));
    if (fused)
        k_dec_batch_gather<<<dim3(4, (unsigned)T), dim3(256), 0, m->stream>>>((const half_t *)m->g[T_EMBD].data, tok_d, pos_d, (int)D, (int)m->g[T_EMBD].rows,
                                                                              m->x, c.rope_order ? m->brope : nullptr, c.head_dim, c.rope_theta,
                                                                              (int)(c.head_dim * c.partial_rotary + 0.5f), c.embd_scale);
    else
        k_gather_rows<<<dim3(4, (unsigned)T), dim3(256), 0, m->stream>>>((const half_t *)m->g[T_EMBD].data, tok_d, T, (int)D,
                                                                          (int)m->g[T_EMBD].rows, m->x, c.embd_scale);
    IFA_LAUNCH_CHECK();
    half_t *x = m->x;
    const Tensor none;
    const bool seq_wiring = !c.parallel_attn && !c.share_input;
    bool xn_ready = false;           // see forward_ops: every residual Add is fused with the norm that follows it
    if (fused) {
        for (int l = 0; l < c.layers; l++) {
            if ((rc = batch_fused_layer(m, R, l, n, x, m->f, rows_d + (size_t)l * (size_t)n, draft))) return rc;
            std::swap(m->x, m->f);
            x = m->x;
        }
    }
    for (int l = fused ? c.layers : 0; l < c.layers; l++) {
        Layer &L = m->layers[(size_t)l];
        const half_t *attn_in = x;
        if (L.t[T_ATTN_NORM].present()) {
            if (!xn_ready && (rc = norm_rows(m, x, T, L.t[T_ATTN_NORM], L.t[T_ATTN_NORM_B], m->xn, c.attn_norm_base))) return rc;
            attn_in = m->xn;
        }
        xn_ready = false;
        if ((rc = matmul(m, attn_in, T, L.t[T_WQ], L.t[T_WQ_B], m->q))) return rc;
        if ((rc = matmul(m, attn_in, T, L.t[T_WK], L.t[T_WK_B], m->k))) return rc;
        if ((rc = matmul(m, attn_in, T, L.t[T_WV], L.t[T_WV_B], m->v))) return rc;
        if (c.rope_order != 0) {
            if ((rc = ifa_rope_rows(m->q, c.head_dim, c.heads, T, pos_d, c.rope_theta, c.rope_order, c.partial_rotary, s))) return rc;
            if ((rc = ifa_rope_rows(m->k, c.head_dim, c.kv_heads, T, pos_d, c.rope_theta, c.rope_order, c.partial_rotary, s))) return rc;
        }
        const AttnRowH *lr = rows_d + (size_t)l * (size_t)n;
        if (c.kv_dtype == Q8_B32T2) k_kv_store_rows<true><<<dim3((unsigned)n, 2), dim3(256), 0, m->stream>>>(m->k, m->v, (int)KVD, m->kv_row_bytes, lr);
        else k_kv_store_rows<false><<<dim3((unsigned)n, 2), dim3(256), 0, m->stream>>>(m->k, m->v, (int)KVD, m->kv_row_bytes, lr);
        IFA_LAUNCH_CHECK();
        if ((rc = ifa_attention_rows(m->q, lr, c.kv_dtype, n, attn_ctx, c.heads, c.kv_heads, c.head_dim, c.use_alibi ? 1.0f : c.kq_scale,
                                     c.use_alibi, c.tp_rank * c.heads, c.heads * std::max(1, c.tp_size), m->att, s))) return rc;
        if ((rc = matmul(m, m->att, T, L.t[T_WO], merging ? none : L.t[T_WO_B], m->a))) return rc;
        if ((rc = tp_merge_rows(m, m->a, T, L.t[T_WO_B]))) return rc;
        if ((rc = layer_tail_ops(m, l, T, x, attn_in, xn_ready))) return rc;
    }
    if (scale_on(c.out_scale) && (rc = ifa_scale(x, c.out_scale, (size_t)T * D, x, s))) return rc;
    const half_t *hfin = x;
    if (m->g[T_OUT_NORM].present()) {
        if (!xn_ready && (rc = norm_rows(m, x, T, m->g[T_OUT_NORM], m->g[T_OUT_NORM_B], m->xn, c.out_norm_base))) return rc;
        hfin = m->xn;
    }
    const Tensor &lm = m->g[T_LM_HEAD];
    const size_t V = lm.rows;
    if ((rc = matmul(m, hfin, T, lm, none, m->logits))) return rc;
    if (logits_out) IFA_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)T * V * 2, hipMemcpyDeviceToDevice, m->stream));
    if (tp) {                // one distributed argmax per row over the group's vocabulary shards
        if ((rc = tp_pick_rows(m, *tp, m->logits, V, (int)V, n))) return rc;
        IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned + 8, m->tp_tok, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
        return IFA_OK;
    }
    if ((rc = ifa_argmax_rows(m->logits, V, V, (size_t)n, m->state + 8, m->state + 3, s))) return rc;      // one launch for the n rows
    if (!fed) IFA_HIP_CHECK(hipMemcpyAsync(m->host_pinned + 8, m->state + 8, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
    };
    if (use_graph) {
        // (forward ops swap m->x / m->f per layer: an odd layer count would leave them exchanged between replays)
        auto it = graphs.find(n);
        if (it == graphs.end()) {
            hipGraphExec_t ex = nullptr;
            if ((rc = capture_graph(m, "batched step", &ex, nullptr, body))) return rc;
            it = graphs.emplace(n, ex).first;
        }
        IFA_HIP_CHECK(hipGraphLaunch(it->second, m->stream));
    } else if ((rc = body())) return rc;
    if (fed) return IFA_OK;
    if (!tp && (rc = tail_enqueue(m, t, cur, m->logits, n))) return rc;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if ((rc = wait_err_check("batched decode step"))) { drop_graphs(m); return rc; }      // (the captured steps hold K-parts launches: re-captured without them)
    if (next_tokens) for (int r = 0; r < n; r++) next_tokens[r] = m->host_pinned[8 + r];
    return IFA_OK;
}

int forward_impl(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev, int *next_token_host,
                 const StepTail &t, TailCursor &cur)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_forward: model not finalized");
    IFA_REQUIRE(tokens_host, "ifa_model_forward: null tokens");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    PromptRoute R;
    int rc = prompt_route_ready(m, n_tokens, prefix_len, true, R);
    if (rc) return rc;
    const size_t V = m->g[T_LM_HEAD].present() ? m->g[T_LM_HEAD].rows : 0;
    if (R.kind == PROMPT_EXACT) {      // order-exact: the tokens one by one through the single-row step (the reference's T = 1 branch for every row)
        for (int i = 0; i < n_tokens; i++) {
            rc = forward_exact(m, tokens_host[i], prefix_len + i, logits_out_dev ? (char *)logits_out_dev + (size_t)i * V * 2 : nullptr,
                               i == n_tokens - 1 ? next_token_host : nullptr, t, cur);
            if (rc) return rc;
        }
        return IFA_OK;
    }
    if (!R.first_pass) return forward_ops(m, tokens_host, n_tokens, prefix_len, logits_out_dev, next_token_host, t, cur, false, &R);
    // Two passes (round 5: 32 tokens, then 2..16 through the rows GEMM, whose weights stream into registers five groups deep, instead of
    // one pass of the op-by-op layer: 40 tokens 7.08 -> 6.35 ms, 48 tokens 7.26 -> 6.67, profiles/r05_prompt_lengths.log; two passes of 17..32
    // rows each -- 49..64 tokens -- measured no faster than the tile kernels).  The second pass reads the first one's K / V rows from the
    // cache like any continued prompt; every row goes through the kernels of a prompt of <= 32 tokens.  Never a one-token pass: a single
    // row takes the int8 GEMV (the reference's rule for ONE row), which is not how a prompt's rows are computed.  Each pass plans itself.
    const int t1 = R.first_pass;
    if ((rc = forward_ops(m, tokens_host, t1, prefix_len, logits_out_dev, nullptr, t, cur, true))) return rc;
    rc = forward_ops(m, tokens_host + t1, n_tokens - t1, prefix_len + t1, logits_out_dev ? (char *)logits_out_dev + (size_t)t1 * V * 2 : nullptr, next_token_host, t, cur);
    m->prompt_route = R;
    return rc;
}

int decode_batch_impl(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host, int *next_tokens_host,
                      void *logits_out_dev, const StepTail &t, TailCursor &cur)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode_batch: model not finalized");
    IFA_REQUIRE(n >= 1 && n <= ifa_model::RING && tokens_host && positions_host && kv_slots_host, "ifa_model_decode_batch: bad arguments");
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    BatchRoute R;
    { int rc = batch_route_ready(m, n, logits_out_dev != nullptr, true, R); if (rc) return rc; }
    if (R.kind == BATCH_EXACT) {      // order-exact: every query's row through the single-row step on ITS cache set (a batched step of the
        // reference is n independent rows; its T > 1 linear branch has no order-exact form here, so the rows go one by one)
        const int back = m->cur_slot;
        const size_t V = m->g[T_LM_HEAD].present() ? m->g[T_LM_HEAD].rows : 0;
        int rc = IFA_OK;
        for (int i = 0; i < n && rc == IFA_OK; i++) {
            if ((rc = ifa_model_select_kv(m, kv_slots_host[i]))) break;
            int nt = 0;
            rc = forward_exact(m, tokens_host[i], positions_host[i], logits_out_dev ? (char *)logits_out_dev + (size_t)i * V * 2 : nullptr, &nt, t, cur);
            if (next_tokens_host) next_tokens_host[i] = nt;
        }
        const int rb = ifa_model_select_kv(m, back);
        return rc ? rc : rb;
    }
    // more queries than the fused five-launch step takes (16): balanced chunks of <= 16, each its own step (the queries are
    // independent; 32 queries op-by-op took 6.7 ms against 2 x 3.1 ms for two fused steps)
    if (R.chunk) {
        for (int c0 = 0; c0 < n; c0++) if (kv_slots_host[c0] < 0) return ifa_fail(IFA_ERR_ARG, "decode_batch: KV slot %d", kv_slots_host[c0]);
        for (int a = 0; a < n; a++)
            for (int b = 0; b < a; b++)
                if (kv_slots_host[a] == kv_slots_host[b]) return ifa_fail(IFA_ERR_ARG, "decode_batch: KV slot %d used twice", kv_slots_host[a]);
        const int per = R.chunk;
        for (int c0 = 0; c0 < n; c0 += per) {
            const int nc = std::min(per, n - c0);
            cur.chunk0 = c0; cur.last_chunk = c0 + nc >= n;
            int rc = forward_batch(m, nc, tokens_host + c0, positions_host + c0, kv_slots_host + c0, next_tokens_host ? next_tokens_host + c0 : nullptr,
                                   logits_out_dev ? (char *)logits_out_dev + (size_t)c0 * m->g[T_LM_HEAD].rows * 2 : nullptr, t, cur);
            if (rc) return rc;
        }
        return IFA_OK;
    }
    return forward_batch(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, logits_out_dev, t, cur);
}

} // namespace ifae

extern "C" {

int ifa_model_forward(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev,
                      int *next_token_host)
{
    StepTail none; TailCursor cur;
    return forward_impl(m, tokens_host, n_tokens, prefix_len, logits_out_dev, next_token_host, none, cur);
}

int ifa_model_decode_batch(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                           int *next_tokens_host, void *logits_out_dev)
{
    StepTail none; TailCursor cur;
    return decode_batch_impl(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, logits_out_dev, none, cur);
}

} // extern "C"
