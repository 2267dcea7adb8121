// ifa_decode_attn256.hip -- the instances of the 256-wide decode attention (ifa_decode_attn256.h) and their launches: what
// launch_attn (ifa_engine_decode.hip) runs for head_dim 256 instead of the generic dispatch.  The P.V and combine launches of the
// split route are the shared kernels instantiated at 256 (their bodies are generic in DG / NSPLIT).  launch_attn256_batch is what
// batch_fused_layer (ifa_engine_forward.hip) runs at this head size for the batched and the draft step.
#include "ifa_engine_state.h"
#include "ifa_decode_attn256.h"

namespace ifae {

template <bool Q8>
static int attn256_go(ifa_model *m, const DecRoute &R, const DecAttnParams &A)
{
    const ifa_model_config &c = m->cfg;
    hipStream_t s = m->stream;
    if (R.kind == DEC_ROUTE_SPLIT) {
        DecAttnSplitWs ws = m->attn_ws; ws.nsplits = R.nsplits;
        const dim3 g2((unsigned)c.heads, (unsigned)R.nsplits);
        int rc;
        if ((rc = launch_lds(k_dec_attn256_scores<Q8>, g2, dim3(256), (size_t)R.lds_scores, s, A, ws))) return rc;
        if ((rc = launch_lds(k_dec_attn_pv<D256, Q8>, g2, dim3(256), (size_t)R.lds_pv, s, A, ws))) return rc;
        return launch_lds(k_dec_attn_combine<D256>, dim3((unsigned)c.heads), dim3(D256), 0, s, ws, m->att.get(), A.xq, c.heads);
    }
    return launch_lds(k_dec_attn256<Q8>, dim3((unsigned)c.heads), dim3(256), (size_t)R.lds_attn, s, A.q, A.kcache, A.vcache, A.heads, A.kv_heads, A);
}

int launch_attn256(ifa_model *m, const DecRoute &R, const DecAttnParams &A)
{
    if (m->cfg.head_dim != D256 || R.kind == DEC_ROUTE_FUSED_TAIL || R.kt || (R.kind == DEC_ROUTE_ONE_WORKGROUP && R.pb != 256))
        return ifa_fail(IFA_ERR_ARG, "fused attention: no 256-wide instance for head_dim %d, route kind %d, %d-row bucket, K tile %d", m->cfg.head_dim, R.kind, R.pb, R.kt);
    return A.kv_q8 ? attn256_go<true>(m, R, A) : attn256_go<false>(m, R, A);
}

// the batched / draft step's attention of n rows (batch_fused_layer: A carries batch_rows, q_stride, skip_store; lds = dec_attn_smem(256, ..))
int launch_attn256_batch(ifa_model *m, int n, size_t lds, const DecAttnParams &A)
{
    if (m->cfg.head_dim != D256 || !A.batch_rows || n < 1)
        return ifa_fail(IFA_ERR_ARG, "batched attention: no 256-wide instance for head_dim %d, %d rows", m->cfg.head_dim, n);
    const dim3 grid((unsigned)m->cfg.heads, (unsigned)n);
    const DecAttnBatchRow *rows = (const DecAttnBatchRow *)A.batch_rows;
    if (A.kv_q8) return launch_lds(k_dec_attn256_batch<true>, grid, dim3(256), lds, m->stream, A.q, rows, A.heads, A.kv_heads, A.q_stride, A);
    return launch_lds(k_dec_attn256_batch<false>, grid, dim3(256), lds, m->stream, A.q, rows, A.heads, A.kv_heads, A.q_stride, A);
}

} // namespace ifae
