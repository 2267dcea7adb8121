// ifa_engine_draft_sampled.hip -- ifa_model_decode_draft_sampled: the draft step of lookup decoding (ifa_model_decode_draft: n rows of
// ONE query in one batched step, the graph captured per n) for a seeded SAMPLED query.  The step itself is ifa_model_decode_draft's,
// launch for launch -- the same captured graph, the same cache rows.  Its tail is TAIL_DRAFT_VERIFY (ifa_engine_state.h): behind the
// replay, on the worker's stream and in front of the call's one synchronisation:
//   [ifa_logit_adjust_draft_rows with the state of state_slot: row r as if draft[0..r) had been counted]
//   -> ifa_topk_pool over the n rows with k = p->pool_size and the mask of ifa_model_set_pool_excluded
//   -> k_sample_verify (csrc/ifa_sample_verify.hip): the rows drawn as a chain, stopping at the first draw that differs from its draft
//   -> one copy of {generator state, n_out, err, tokens} into pinned staging.
// What differs from call to call -- parameters, state slot, draft tokens, generator state -- lives in device memory (m->draft_blk) and
// is written by the call, as ifa_model_decode_sampled does it.  Nothing here is captured; the greedy, draft and sampled graphs are
// not touched.  The call never writes the logit state: the caller counts the tokens it emits.
#include <algorithm>
#include "ifa_engine_state.h"
#include "ifa_sample_rule.h"

namespace ifa {
int logit_adjust_draft_rows(const void *logits, size_t row_stride, const int *state_slot_dev, size_t rows, size_t n, const int *draft_dev,
                            const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s);
int sample_verify_launch(const int *counts, const int *ids, const void *vals, int rows, int k_stride, const ifa_sample_params *params, const int *draft,
                         unsigned long long *rng, int *tokens_out, int *index_out, int *n_out, int *err, hipStream_t s);
}

namespace ifae {

int draft_sampled_enqueue(ifa_model *m, const StepTail &t, const half_t *logits, int n)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    hipStream_t s = m->stream;
    DraftBlk *blk = m->draft_blk.dev;
    int rc;
    const half_t *src = logits;
    if (t.armed) {      // (its own kernel: row r as if draft[0..r) had been counted)
        if ((rc = ifa::logit_adjust_draft_rows(logits, V, &blk->slot, (size_t)n, V, blk->draft, m->la_state, m->la_bias, m->la_params, m->la_adj, s))) return rc;
        src = m->la_adj;
    }
    const PoolBlock B = pool_block(m->pool_blk.dev.get(), n, t.k, false);
    if ((rc = pool_rows_launch(m, B, t.k, src, nullptr, nullptr, 0, n))) return rc;
    if ((rc = ifa::sample_verify_launch(B.counts, B.ids, B.vals, n, t.k, &blk->p, blk->draft, &blk->rng, blk->tokens, nullptr, &blk->n_out, &blk->err, s))) return rc;
    constexpr size_t off = offsetof(DraftBlk, rng);
    IFA_HIP_CHECK(hipMemcpyAsync((char *)m->draft_blk.pin.get() + off, (const char *)blk + off, offsetof(DraftBlk, back_end) - off, hipMemcpyDeviceToHost, s));
    return IFA_OK;
}

} // namespace ifae

extern "C" int ifa_model_decode_draft_sampled(ifa_model *m, int n, const int *tokens_host, int pos0, const ifa_sample_params *p,
                                              unsigned long long *rng_state_inout, int state_slot, int *out_tokens_host, int *n_out)
{
    using namespace ifae;
    const char *who = "ifa_model_decode_draft_sampled";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(tokens_host && p && rng_state_inout && out_tokens_host && n_out, "%s: null pointer", who);
    IFA_REQUIRE(n >= 2 && n <= 8, "%s: %d rows (2..8: the committed token and 1..7 draft tokens)", who, n);
    IFA_REQUIRE(pos0 >= 0 && (long long)pos0 + n <= (long long)m->cfg.max_ctx, "%s: rows %d..%d outside max_ctx %d", who, pos0, pos0 + n - 1, m->cfg.max_ctx);
    IFA_REQUIRE(ifa_sr::sr_strategy_ok(p->strategy_id), "%s: strategy %d is not one of 1 sample.std, 2 greedy, 3 top_k, 4 sample.top_p, 7 min_p", who, p->strategy_id);
    IFA_REQUIRE(p->pool_size >= 1 && p->pool_size <= IFA_POOL_MAX, "%s: pool_size %d outside 1..%d", who, p->pool_size, IFA_POOL_MAX);
    int rc = device_tail_refusals(m, who, true, true, "take ifa_model_decode_sampled");
    if (rc) return rc;
    IFA_REQUIRE(state_slot >= -1 && (state_slot < 0 || (size_t)state_slot < m->la_slots), "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, state_slot);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    // everything the tail allocates, outside any capture
    if (!m->draft_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->draft_blk.reserve(1))) return rc;
    }
    if ((rc = pool_reserve(m, n, p->pool_size))) return rc;
    if (state_slot >= 0 && (rc = la_adj_reserve(m, 8, who))) return rc;
    // the call's values into device memory, in front of the step
    DraftBlk *pin = m->draft_blk.pin;
    memset(pin, 0, sizeof(DraftBlk));
    pin->p = *p;
    pin->slot = std::max(state_slot, 0);
    for (int i = 0; i + 1 < n; i++) pin->draft[i] = tokens_host[i + 1];      // draft[i]: the guess for the token row i emits
    pin->rng = *rng_state_inout;
    IFA_HIP_CHECK(hipMemcpyAsync(m->draft_blk.dev, pin, sizeof(DraftBlk), hipMemcpyHostToDevice, m->stream));
    StepTail t; TailCursor cur;
    t.kind = TAIL_DRAFT_VERIFY; t.k = p->pool_size; t.armed = state_slot >= 0;
    int pos[8], slot[8];
    for (int i = 0; i < n; i++) { pos[i] = pos0 + i; slot[i] = m->cur_slot; }
    if ((rc = forward_batch(m, n, tokens_host, pos, slot, nullptr, nullptr, t, cur, true))) return rc;
    // behind the step's synchronisation
    if (pin->err != 0)
        return ifa_fail(IFA_ERR_STATE, "%s: row %d had no token to draw (an empty candidate pool); the results of this call are not valid", who, pin->err - 1);
    const int e = pin->n_out;
    if (e < 1 || e > n) return ifa_fail(IFA_ERR_STATE, "%s: the verify step emitted %d of %d tokens", who, e, n);
    *rng_state_inout = pin->rng;
    for (int i = 0; i < n; i++) out_tokens_host[i] = pin->tokens[i];
    *n_out = e;
    return IFA_OK;
}
