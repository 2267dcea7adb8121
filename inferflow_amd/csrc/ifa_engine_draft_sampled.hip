// ifa_engine_draft_sampled.hip -- ifa_model_decode_draft_sampled: the draft step of lookup decoding (ifa_model_decode_draft: n rows of
// ONE query in one batched step, the graph captured per n) for a seeded SAMPLED query.  The step itself is ifa_model_decode_draft's,
// launch for launch -- the same captured graph, the same cache rows.  Behind its replay, on the worker's stream and in front of the
// call's one synchronisation:
//   [ifa_logit_adjust_draft_rows with the state of state_slot: row r as if draft[0..r) had been counted]
//   -> ifa_topk_pool over the n rows with k = p->pool_size and the mask of ifa_model_set_pool_excluded
//   -> k_sample_verify (csrc/ifa_sample_verify.hip): the rows drawn as a chain, stopping at the first draw that differs from its draft
//   -> one copy of {generator state, n_out, err, tokens} into pinned staging.
// What differs from call to call -- parameters, state slot, draft tokens, generator state -- lives in device memory (m->dsv_blk) and
// is written by the call, as ifa_model_decode_sampled does it.  Nothing here is captured; the greedy, draft and sampled graphs are
// not touched.  The call never writes the logit state: the caller counts the tokens it emits.
#include <algorithm>
#include "ifa_engine_state.h"
#include "ifa_sample_rule.h"

namespace ifa {
int topk_pool_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, int k, const unsigned *excl,
                   int *ids_out, void *vals_out, int *count_out, hipStream_t s);
int logit_adjust_draft_rows(const void *logits, size_t row_stride, const int *state_slot_dev, size_t rows, size_t n, const int *draft_dev,
                            const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s);
int sample_verify_launch(const int *counts, const int *ids, const void *vals, int rows, int k_stride, const ifa_sample_params *params, const int *draft,
                         unsigned long long *rng, int *tokens_out, int *index_out, int *n_out, int *err, hipStream_t s);
}

namespace ifae {

// m->dsv_blk, in ints: what the call uploads [0, DB_RNG + 2), what comes back [DB_RNG, DB_BACK_END)
enum { DB_PARAMS = 0, DB_SLOT = 6, DB_DRAFT = 8, DB_RNG = 16, DB_NOUT = 18, DB_ERR = 19, DB_TOKENS = 20, DB_BACK_END = 28, DB_WORDS = 32 };
static_assert(sizeof(ifa_sample_params) <= DB_SLOT * sizeof(int), "ifa_sample_params outgrew its words of the block");

int draft_sampled_enqueue(ifa_model *m, const half_t *logits, int n)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    const int k = m->dsv.k;
    hipStream_t s = m->stream;
    int *blk = m->dsv_blk.dev;
    int rc;
    const half_t *src = logits;
    if (m->dsv.armed) {
        if ((rc = ifa::logit_adjust_draft_rows(logits, V, blk + DB_SLOT, (size_t)n, V, blk + DB_DRAFT, m->la_state, m->la_bias, m->la_params, m->la_adj, s))) return rc;
        src = m->la_adj;
    }
    int *counts = (int *)m->pool_blk.dev.get(), *ids = counts + n;
    uint16_t *vals = (uint16_t *)(ids + (size_t)n * k);
    if ((rc = ifa::topk_pool_rows(src, V, nullptr, (size_t)n, V, k, m->pool_excl, ids, vals, counts, s))) return rc;
    if ((rc = ifa::sample_verify_launch(counts, ids, vals, n, k, (const ifa_sample_params *)(blk + DB_PARAMS), blk + DB_DRAFT,
                                        (unsigned long long *)(blk + DB_RNG), blk + DB_TOKENS, nullptr, blk + DB_NOUT, blk + DB_ERR, s))) return rc;
    IFA_HIP_CHECK(hipMemcpyAsync(m->dsv_blk.pin + DB_RNG, blk + DB_RNG, sizeof(int) * (DB_BACK_END - DB_RNG), hipMemcpyDeviceToHost, s));
    return IFA_OK;
}

// disarms on every way out
struct DsvDisarm { ifa_model *m; ~DsvDisarm() { m->dsv = ifa_model::DraftSampReq(); } };

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
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "%s: partitioned workers have no draft step", who);
    if (!m->g[T_LM_HEAD].present() || !m->g[T_EMBD].present()) return ifa_fail(IFA_ERR_STATE, "%s: embeddings / lm_head missing (pipeline stage worker)", who);
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "%s: option exact_order steps one row at a time; take ifa_model_decode_sampled", who);
    if (m->opt_perf_stat) return ifa_fail(IFA_ERR_STATE, "%s: option perf_stat times the single-row step; take ifa_model_decode_sampled", who);
    IFA_REQUIRE(state_slot >= -1 && (state_slot < 0 || (size_t)state_slot < m->la_slots), "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, state_slot);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    // everything the tail allocates, outside any capture
    const size_t V = m->g[T_LM_HEAD].rows;
    int rc;
    if (!m->dsv_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->dsv_blk.reserve(DB_WORDS))) return rc;
    }
    if ((rc = pool_reserve(m, n, p->pool_size))) return rc;
    if (state_slot >= 0 && 8 * V > m->la_adj.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if (m->la_adj.alloc(8 * V)) return ifa_fail(IFA_ERR_NOMEM, "%s: no memory for the adjusted logits rows", who);
    }
    // the call's values into device memory, in front of the step
    int *pin = m->dsv_blk.pin;
    memset(pin, 0, sizeof(int) * DB_WORDS);
    memcpy(pin + DB_PARAMS, p, sizeof(ifa_sample_params));
    pin[DB_SLOT] = std::max(state_slot, 0);
    for (int i = 0; i + 1 < n; i++) pin[DB_DRAFT + i] = tokens_host[i + 1];      // draft[i]: the guess for the token row i emits
    memcpy(pin + DB_RNG, rng_state_inout, sizeof(unsigned long long));
    IFA_HIP_CHECK(hipMemcpyAsync(m->dsv_blk.dev, pin, sizeof(int) * DB_WORDS, hipMemcpyHostToDevice, m->stream));
    DsvDisarm disarm{m};
    m->dsv.k = p->pool_size; m->dsv.armed = state_slot >= 0;
    int pos[8], slot[8];
    for (int i = 0; i < n; i++) { pos[i] = pos0 + i; slot[i] = m->cur_slot; }
    if ((rc = forward_batch(m, n, tokens_host, pos, slot, nullptr, nullptr, true))) return rc;
    // behind the step's synchronisation
    if (pin[DB_ERR] != 0)
        return ifa_fail(IFA_ERR_STATE, "%s: row %d had no token to draw (an empty candidate pool); the results of this call are not valid", who, pin[DB_ERR] - 1);
    const int e = pin[DB_NOUT];
    if (e < 1 || e > n) return ifa_fail(IFA_ERR_STATE, "%s: the verify step emitted %d of %d tokens", who, e, n);
    memcpy(rng_state_inout, pin + DB_RNG, sizeof(unsigned long long));
    for (int i = 0; i < n; i++) out_tokens_host[i] = pin[DB_TOKENS + i];
    *n_out = e;
    return IFA_OK;
}
