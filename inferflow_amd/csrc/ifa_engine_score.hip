// ifa_engine_score.hip -- a prompt that ends in log-probabilities instead of a logits block (ifa_model_forward_score): a TAIL_SCORE
// tail (ifa_engine_state.h) over the prompt's n rows.  With it the lm_head runs over ALL rows into the worker's own m->logits, exactly
// as it does for a caller's logits_out_dev, and every route the prompt takes (one pass, the two passes of a 34..48-token prompt,
// exact_order's row-by-row steps, perf_stat's op-by-op layer) serves the rows it has just written: the row log-sum-exp + target gather
// (csrc/ifa_logprob.hip) and, behind the last row, ONE copy of 2 * n floats into pinned staging, all in front of that route's
// synchronisation.  No [T][vocab] block leaves the worker.
#include "ifa_engine_state.h"

namespace ifa {
int lse_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, const int *targets_dev, float *lse_out,
             float *target_out, float *part_dev, hipStream_t s);
}

namespace ifae {

int lse_part_reserve(ifa_model *m)
{
    return m->lse_part ? IFA_OK : m->lse_part.alloc(LSE_PART_FLOATS);
}

// staging for n rows (grown on demand, outside any step)
static int score_reserve(ifa_model *m, int n)
{
    int rc = lse_part_reserve(m);
    if (rc) return rc;
    // (score_out, grown last, answers for both pairs: a failure in either leaves it empty)
    if (2 * (size_t)n <= m->score_out.cap()) return IFA_OK;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    const size_t cap = (size_t)std::max(n, 64);
    m->score_out.reset(); m->score_tgt.reset();
    if ((rc = m->score_tgt.reserve(cap)) || (rc = m->score_out.reserve(2 * cap))) return rc;
    return IFA_OK;
}

int score_enqueue(ifa_model *m, const StepTail &t, TailCursor &cur, const half_t *logits, int n_rows)
{
    if (n_rows <= 0 || cur.done + n_rows > t.n) return ifa_fail(IFA_ERR_STATE, "score: a step of %d rows after %d of %d", n_rows, cur.done, t.n);
    const size_t V = m->g[T_LM_HEAD].rows;
    // lse [n] | target logit [n]: the parts of a prompt taken in several steps land side by side
    int rc = lse_rows(logits, V, nullptr, (size_t)n_rows, V, m->score_tgt.dev + cur.done, m->score_out.dev + cur.done, m->score_out.dev + t.n + cur.done,
                      m->lse_part, m->stream);
    if (rc) return rc;
    cur.done += n_rows;
    if (cur.done == t.n)
        IFA_HIP_CHECK(hipMemcpyAsync(m->score_out.pin, m->score_out.dev, sizeof(float) * 2 * (size_t)t.n, hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

} // namespace ifae

extern "C" {

int ifa_model_forward_score(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, const int *targets_host,
                            float *lse_host, float *target_logit_host, int *next_token_host)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_forward_score: model not finalized");
    IFA_REQUIRE(tokens_host && n_tokens >= 1 && targets_host && lse_host && target_logit_host, "ifa_model_forward_score: bad arguments");
    int rc = device_tail_refusals(m, "ifa_model_forward_score", false, false, "score on the host there");
    if (rc) return rc;
    const size_t V = m->g[T_LM_HEAD].rows;
    for (int i = 0; i < n_tokens; i++)
        IFA_REQUIRE(targets_host[i] < 0 || (size_t)targets_host[i] < V, "ifa_model_forward_score: target %d outside the vocabulary", targets_host[i]);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    if ((rc = score_reserve(m, n_tokens))) return rc;
    memcpy(m->score_tgt.pin, targets_host, sizeof(int) * (size_t)n_tokens);
    IFA_HIP_CHECK(hipMemcpyAsync(m->score_tgt.dev, m->score_tgt.pin, sizeof(int) * (size_t)n_tokens, hipMemcpyHostToDevice, m->stream));
    StepTail t; TailCursor cur;
    t.kind = TAIL_SCORE; t.n = n_tokens;
    int next = -1;
    if ((rc = forward_impl(m, tokens_host, n_tokens, prefix_len, nullptr, &next, t, cur))) return rc;
    if (cur.done != t.n) return ifa_fail(IFA_ERR_STATE, "ifa_model_forward_score: the prompt served %d of %d rows", cur.done, t.n);
    memcpy(lse_host, m->score_out.pin, sizeof(float) * (size_t)n_tokens);
    memcpy(target_logit_host, m->score_out.pin + n_tokens, sizeof(float) * (size_t)n_tokens);
    if (next_token_host) *next_token_host = next;
    return IFA_OK;
}

} // extern "C"
