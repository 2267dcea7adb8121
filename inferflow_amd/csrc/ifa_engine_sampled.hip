// ifa_engine_sampled.hip -- ifa_model_decode_sampled: the fused decode step replayed per token like ifa_model_decode, with the
// token DRAWN on the device instead of taken greedily.  The captured step gathers its own input and ends in
//   lm_head -> [logit processors of the query's state slot] -> candidate pool (k_topk_pool) -> draw + state advance (k_sample_pool)
//   -> [one more occurrence of the drawn token in the state slot]
// all plain launches on the worker's stream.  What differs from call to call -- the strategy's parameters, the generator state, the
// state slot, the error word -- lives in device memory (m->samp_blk) and is written by the call, like m->state: nothing of it is
// a kernel argument of a captured launch.  The greedy step, its graphs and its kernels are not touched: the sampled step has exec
// handles of its own, keyed by what IS baked into its launches (KV slot, pool length, processors armed, the buffers' addresses).
#include <algorithm>
#include "ifa_engine_state.h"
#include "ifa_sample_rule.h"

namespace ifa {
int topk_pool_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, int k, const unsigned *excl,
                   int *ids_out, void *vals_out, int *count_out, hipStream_t s);
int logit_adjust_rows(const void *logits, size_t row_stride, const int *row_idx_dev, const int *state_slot_dev, size_t rows, size_t n,
                      const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s);
int sample_pool_launch(const int *counts, const int *ids, const void *vals, size_t rows, int k_stride, const ifa_sample_params *params,
                       unsigned long long *rng, int *tokens_out, int *index_out, float *weights_out, int *err, int *state, int ring, hipStream_t s);
}

namespace ifae {

// m->samp_blk, in ints: the call's block in device memory and its pinned twin
enum { SB_PARAMS = 0, SB_RNG = 6, SB_SLOT = 8, SB_ERR = 9, SB_TOKEN = 10, SB_INDEX = 11, SB_WORDS = 16 };
static_assert(sizeof(ifa_sample_params) <= SB_RNG * sizeof(int), "ifa_sample_params outgrew its words of the block");

// everything the sampled step allocates, outside any capture; the call's k / armed for the launches
int sampled_prepare(ifa_model *m, const SampledCall &sc)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    int rc;
    if (!m->samp_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->samp_blk.reserve(SB_WORDS))) return rc;
    }
    if ((rc = pool_reserve(m, 1, sc.p->pool_size))) return rc;
    if (sc.state_slot >= 0 && V > m->la_adj.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if (m->la_adj.alloc(8 * V)) return ifa_fail(IFA_ERR_NOMEM, "ifa_model_decode_sampled: no memory for the adjusted logits row");
    }
    m->samp_k = sc.p->pool_size; m->samp_armed = sc.state_slot >= 0;
    return IFA_OK;
}

// the end of a sampled step (under capture or not): m->samp_k / m->samp_armed are what the call set
int sampled_tail_enqueue(ifa_model *m, const half_t *x)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    const int k = m->samp_k;
    hipStream_t s = m->stream;
    int *blk = m->samp_blk.dev;
    int rc;
    if ((rc = launch_lm(m, x))) return rc;
    const half_t *src = m->logits;
    if (m->samp_armed) {
        if ((rc = ifa::logit_adjust_rows(m->logits, V, nullptr, blk + SB_SLOT, 1, V, m->la_state, m->la_bias, m->la_params, m->la_adj, s))) return rc;
        src = m->la_adj;
    }
    int *counts = (int *)m->pool_blk.dev.get(), *ids = counts + 1;
    uint16_t *vals = (uint16_t *)(ids + k);
    if ((rc = ifa::topk_pool_rows(src, V, nullptr, 1, V, k, m->pool_excl, ids, vals, counts, s))) return rc;
    if ((rc = ifa::sample_pool_launch(counts, ids, vals, 1, k, (const ifa_sample_params *)(blk + SB_PARAMS), (unsigned long long *)(blk + SB_RNG),
                                      blk + SB_TOKEN, blk + SB_INDEX, nullptr, blk + SB_ERR, m->state, ifa_model::RING, s))) return rc;
    // the drawn token is state[0] now: counted before the next step's adjust reads the slot
    if (m->samp_armed && (rc = ifa_logit_state_add(blk + SB_SLOT, m->state, 1, V, m->la_slots, m->la_state, (ifa_stream)s))) return rc;
    return IFA_OK;
}

// the captured sampled step of the selected KV slot for (k, armed); re-captured when a buffer it names has moved
int sampled_graph(ifa_model *m, hipGraphExec_t *exec_out)
{
    const int key = (m->cur_slot << 10) | (m->samp_k << 1) | (m->samp_armed ? 1 : 0);
    ifa_model::SampGraph &G = m->samp_graphs[key];
    const void *now[8] = {m->samp_blk.dev.get(), m->pool_blk.dev.get(), m->pool_excl.get(), m->la_state.get(), m->la_bias.get(), m->la_params.get(),
                          m->la_adj.get(), m->logits};
    if (G.exec && !std::equal(now, now + 8, G.ptrs)) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
    if (!G.exec) {
        hipStream_t s = m->stream;
        IFA_HIP_CHECK(hipStreamSynchronize(s));
        IFA_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_fused_step(m, STEP_TAIL_SAMPLED);
        hipGraph_t gph = nullptr;
        const hipError_t e = hipStreamEndCapture(s, &gph);
        if (rc) { if (gph) (void)hipGraphDestroy(gph); return rc; }
        if (e != hipSuccess) return ifa_fail(IFA_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        const hipError_t ei = hipGraphInstantiate(&G.exec, gph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gph);
        if (ei != hipSuccess) { G.exec = nullptr; return ifa_fail(IFA_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ei)); }
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
    int *pin = m->samp_blk.pin;
    memset(pin, 0, sizeof(int) * SB_WORDS);
    memcpy(pin + SB_PARAMS, sc.p, sizeof(ifa_sample_params));
    memcpy(pin + SB_RNG, sc.rng, sizeof(unsigned long long));
    pin[SB_SLOT] = std::max(sc.state_slot, 0);
    IFA_HIP_CHECK(hipMemcpyAsync(m->samp_blk.dev, pin, sizeof(int) * SB_WORDS, hipMemcpyHostToDevice, m->stream));
    return IFA_OK;
}

// behind the last step, in front of the call's one synchronisation
int sampled_copy_back(ifa_model *m)
{
    IFA_HIP_CHECK(hipMemcpyAsync(m->samp_blk.pin + SB_RNG, m->samp_blk.dev + SB_RNG, sizeof(int) * (SB_WORDS - SB_RNG), hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

// after the synchronisation: the generator state goes back to the caller; a step that had nothing to draw from fails the call
int sampled_finish(ifa_model *m, const SampledCall &sc)
{
    const int *pin = m->samp_blk.pin;
    if (pin[SB_ERR] != 0)
        return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_sampled: step %d had no token to draw (an empty candidate pool); the results of this call are not valid", pin[SB_ERR] - 1);
    memcpy(sc.rng, pin + SB_RNG, sizeof(unsigned long long));
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
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "%s: the vocabulary of a partitioned worker is sharded; the draw runs on a single-device worker", who);
    if (!m->g[T_LM_HEAD].present() || !m->g[T_EMBD].present()) return ifa_fail(IFA_ERR_STATE, "%s: embeddings / lm_head missing (pipeline stage worker)", who);
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "%s: option exact_order steps on the host; the sampled step is the fused, captured one", who);
    if (m->opt_perf_stat) return ifa_fail(IFA_ERR_STATE, "%s: option perf_stat times the op-by-op step; the sampled step is the fused, captured one", who);
    std::string why;
    if (!m->opt_fused || !fused_supported(m, &why)) return ifa_fail(IFA_ERR_STATE, "%s: the fused decode step does not cover this model (%s)", who, m->opt_fused ? why.c_str() : "option fused = 0");
    IFA_REQUIRE(state_slot >= -1 && (state_slot < 0 || (size_t)state_slot < m->la_slots), "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, state_slot);
    SampledCall sc;
    sc.p = p; sc.rng = rng_state_inout; sc.state_slot = state_slot;
    return decode_impl(m, first_token, start_pos, n_steps, out_tokens_host, elapsed_ms, false, &sc);
}

} // extern "C"
