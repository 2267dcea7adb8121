// ifa_engine_sampled.hip -- ifa_model_decode_sampled: the fused decode step replayed per token like ifa_model_decode, with the
// token DRAWN on the device instead of taken greedily.  The captured step gathers its own input and ends in
//   lm_head -> [logit processors of the query's state slot] -> candidate pool (k_topk_pool) -> draw + state advance (k_sample_pool)
//   -> [one more occurrence of the drawn token in the state slot]
// all plain launches on the worker's stream: a TAIL_SAMPLED tail (ifa_engine_state.h), the one kind that runs INSIDE the step and is
// captured with it.  What differs from call to call -- the strategy's parameters, the generator state, the
// state slot, the error word -- lives in device memory (m->samp_blk) and is written by the call, like m->state: nothing of it is
// a kernel argument of a captured launch.  The greedy step, its graphs and its kernels are not touched: the sampled step has exec
// handles of its own, keyed by what IS baked into its launches (KV slot, the tail's pool length and "processors armed", the buffers' addresses).
#include <algorithm>
#include "ifa_engine_state.h"
#include "ifa_sample_rule.h"

namespace ifa {
int sample_pool_launch(const int *counts, const int *ids, const void *vals, size_t rows, int k_stride, const ifa_sample_params *params,
                       unsigned long long *rng, int *tokens_out, int *index_out, float *weights_out, int *err, int *state, int ring, hipStream_t s);
}

namespace ifae {

// everything the sampled step allocates, outside any capture
int sampled_prepare(ifa_model *m, const StepTail &t)
{
    int rc;
    if (!m->samp_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->samp_blk.reserve(1))) return rc;
    }
    if ((rc = pool_reserve(m, 1, t.k))) return rc;
    if (t.armed && (rc = la_adj_reserve(m, 1, "ifa_model_decode_sampled"))) return rc;
    return IFA_OK;
}

// the end of a sampled step (under capture or not): t.k / t.armed are baked into its launches
int sampled_tail_enqueue(ifa_model *m, const StepTail &t, const half_t *x)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    hipStream_t s = m->stream;
    SampBlk *blk = m->samp_blk.dev;
    int rc;
    if ((rc = launch_lm(m, x))) return rc;
    const PoolBlock B = pool_block(m->pool_blk.dev.get(), 1, t.k, false);
    if ((rc = pool_rows_launch(m, B, t.k, m->logits, nullptr, t.armed ? &blk->slot : nullptr, 0, 1))) return rc;
    if ((rc = ifa::sample_pool_launch(B.counts, B.ids, B.vals, 1, t.k, &blk->p, &blk->rng, &blk->token, &blk->index, nullptr, &blk->err, m->state, ifa_model::RING, s))) return rc;
    // the drawn token is state[0] now: counted before the next step's adjust reads the slot
    if (t.armed && (rc = ifa_logit_state_add(&blk->slot, m->state, 1, V, m->la_slots, m->la_state, (ifa_stream)s))) return rc;
    return IFA_OK;
}

// the captured sampled step of the selected KV slot for (k, armed); re-captured when a buffer it names has moved
int sampled_graph(ifa_model *m, const StepTail &t, hipGraphExec_t *exec_out)
{
    const int key = (m->cur_slot << 10) | (t.k << 1) | (t.armed ? 1 : 0);
    ifa_model::SampGraph &G = m->samp_graphs[key];
    const void *now[8] = {m->samp_blk.dev.get(), m->pool_blk.dev.get(), m->pool_excl.get(), m->la_state.get(), m->la_bias.get(), m->la_params.get(),
                          m->la_adj.get(), m->logits};
    if (G.exec && !std::equal(now, now + 8, G.ptrs)) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
    if (!G.exec) {
        const int rc = capture_graph(m, "sampled step", &G.exec, nullptr, [&] { return enqueue_fused_step(m, t); });
        if (rc) return rc;
        std::copy(now, now + 8, G.ptrs);
    }
    *exec_out = G.exec;
    return IFA_OK;
}

void sampled_drop_graphs(ifa_model *m)
{
    for (auto &kv : m->samp_graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    m->samp_graphs.clear();
}

// the call's values into device memory, in front of its first step
int sampled_begin(ifa_model *m, const SampledCall &sc)
{
    SampBlk *pin = m->samp_blk.pin;
    memset(pin, 0, sizeof(SampBlk));
    pin->p = *sc.p; pin->rng = *sc.rng;
    pin->slot = std::max(sc.state_slot, 0);
    IFA_HIP_CHECK(hipMemcpyAsync(m->samp_blk.dev, pin, sizeof(SampBlk), hipMemcpyHostToDevice, m->stream));
    return IFA_OK;
}

// behind the last step, in front of the call's one synchronisation: [rng, end)
int sampled_copy_back(ifa_model *m)
{
    constexpr size_t off = offsetof(SampBlk, rng);
    IFA_HIP_CHECK(hipMemcpyAsync((char *)m->samp_blk.pin.get() + off, (const char *)m->samp_blk.dev.get() + off, sizeof(SampBlk) - off, hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

// after the synchronisation: the generator state goes back to the caller; a step that had nothing to draw from fails the call
int sampled_finish(ifa_model *m, const SampledCall &sc)
{
    const SampBlk *pin = m->samp_blk.pin;
    if (pin->err != 0)
        return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_sampled: step %d had no token to draw (an empty candidate pool); the results of this call are not valid", pin->err - 1);
    *sc.rng = pin->rng;
    return IFA_OK;
}

} // namespace ifae

extern "C" {

int ifa_model_decode_sampled(ifa_model *m, int first_token, int start_pos, int n_steps, const ifa_sample_params *p,
                             unsigned long long *rng_state_inout, int state_slot, int *out_tokens_host, float *elapsed_ms)
{
    using namespace ifae;
    const char *who = "ifa_model_decode_sampled";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(p && rng_state_inout, "%s: null pointer", who);
    IFA_REQUIRE(ifa_sr::sr_strategy_ok(p->strategy_id), "%s: strategy %d is not one of 1 sample.std, 2 greedy, 3 top_k, 4 sample.top_p, 7 min_p", who, p->strategy_id);
    IFA_REQUIRE(p->pool_size >= 1 && p->pool_size <= IFA_POOL_MAX, "%s: pool_size %d outside 1..%d", who, p->pool_size, IFA_POOL_MAX);
    int rc = device_tail_refusals(m, who, true, true, "the sampled step is the fused, captured one of a single-device worker");
    if (rc) return rc;
    std::string why;
    if (!m->opt_fused || !fused_supported(m, &why)) return ifa_fail(IFA_ERR_STATE, "%s: the fused decode step does not cover this model (%s)", who, m->opt_fused ? why.c_str() : "option fused = 0");
    IFA_REQUIRE(state_slot >= -1 && (state_slot < 0 || (size_t)state_slot < m->la_slots), "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, state_slot);
    SampledCall sc;
    sc.p = p; sc.rng = rng_state_inout; sc.state_slot = state_slot;
    StepTail t; TailCursor cur;
    t.kind = TAIL_SAMPLED; t.k = p->pool_size; t.armed = state_slot >= 0; t.sampled = &sc;
    return decode_impl(m, first_token, start_pos, n_steps, out_tokens_host, elapsed_ms, false, t, cur);
}

} // extern "C"
