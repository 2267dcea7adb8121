// ifa_engine_batch_steps.hip -- ifa_model_decode_batch_steps: n_steps batched decode steps of the same n rows with one
// synchronisation.  The tables of the first step -- token, position and per layer (K cache, V cache, context) of every row -- go to
// the device once; every step then is
//   replay of the batched step captured WITHOUT its table upload and copy back (forward_batch, FED_*: the same body, so the
//     launches are those of ifa_model_decode_batch)
//   -> [logit processors of the pooled rows' state slots -> candidate pools (the launches of pool_enqueue) -> clamp of the counts to
//      each row's own pool length -> draw (k_sample_pool)]                                       (only with a row that is not plainly greedy)
//   -> feed (csrc/ifa_batch_feed.hip): token per row, stop ids, ring, token / position / context of every live row + 1
//   -> [one more occurrence of every emitted token in its row's state slot]
// all plain launches on the worker's stream behind the replay, as pool_enqueue's are today.  What differs from call to call lives in
// device memory (m->bs_blk) written by the call; the step number too.  The other entry points' graphs are not touched.
#include <algorithm>
#include <string>
#include <vector>
#include "ifa_engine_state.h"
#include "ifa_sample_rule.h"
#include "ifa_batch_feed.h"

namespace ifa {
int sample_pool_launch(const int *counts, const int *ids, const void *vals, size_t rows, int k_stride, const ifa_sample_params *params,
                       unsigned long long *rng, int *tokens_out, int *index_out, float *weights_out, int *err, int *state, int ring, hipStream_t s);
}

namespace ifae {

// m->bs_blk, in ints.  [0, BS_RING + n_steps * n) comes back in the call's one copy.
constexpr int BS_N = IFA_BATCH_ROWS_MAX, BS_ROW_WORDS = (int)(sizeof(ifa_batch_feed_row) / sizeof(int));
enum { BS_ROWS = 0, BS_STEP = BS_ROWS + BS_N * BS_ROW_WORDS, BS_ERR, BS_DRAW_ERR, BS_PAD, BS_RING,
       BS_PARAMS = BS_RING + IFA_BATCH_STEPS_MAX * BS_N, BS_RNG = BS_PARAMS + BS_N * 6, BS_POOL_LEN = BS_RNG + BS_N * 2,
       BS_DRAWN = BS_POOL_LEN + BS_N, BS_INDEX = BS_DRAWN + BS_N, BS_PAIR_SLOT = BS_INDEX + BS_N, BS_PAIR_TOK = BS_PAIR_SLOT + BS_N,
       BS_WORDS = BS_PAIR_TOK + BS_N };
static_assert(sizeof(ifa_sample_params) == 6 * sizeof(int) && BS_RNG % 2 == 0 && BS_ROWS % 2 == 0, "the block's 8-byte words are aligned");

struct PoolFedGuard { ifa_model *m; ~PoolFedGuard() { pool_fed_end(m); } };

static bool row_pooled(const ifa_batch_row &r) { return r.p.strategy_id != ifa_sr::SR_GREEDY || r.state_slot >= 0; }

} // namespace ifae

extern "C" {

int ifa_model_batch_steps_rows(ifa_model *m)
{
    using namespace ifae;
    if (!m || !m->finalized || m->cfg.tp_size > 1 || m->topo || !m->g[T_LM_HEAD].present() || !m->g[T_EMBD].present() || m->opt_exact_order || m->opt_perf_stat) return 0;
    for (int n : {IFA_BATCH_ROWS_MAX, 16, 2}) {
        BatchRoute R;
        if (batch_route_of_call(m, n, R) == IFA_OK && !R.chunk && R.kind == BATCH_FUSED && R.captured) return n;
    }
    return 0;
}

int ifa_model_decode_batch_steps(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                                 int n_steps, ifa_batch_row *rows, int *out_tokens_host, int *emitted_host, float *elapsed_ms)
{
    using namespace ifae;
    const char *who = "ifa_model_decode_batch_steps";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(n >= 1 && tokens_host && positions_host && kv_slots_host && out_tokens_host && emitted_host, "%s: bad arguments", who);
    IFA_REQUIRE(n_steps >= 1 && n_steps <= IFA_BATCH_STEPS_MAX, "%s: n_steps %d outside 1..%d", who, n_steps, IFA_BATCH_STEPS_MAX);
    // ---- the route: one fused, captured step or nothing
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "%s: a partitioned worker steps through its group; the device-fed steps run on a single-device worker", who);
    if (!m->g[T_LM_HEAD].present() || !m->g[T_EMBD].present()) return ifa_fail(IFA_ERR_STATE, "%s: embeddings / lm_head missing (pipeline stage worker)", who);
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "%s: option exact_order steps the rows one by one on the host", who);
    if (m->opt_perf_stat) return ifa_fail(IFA_ERR_STATE, "%s: option perf_stat times the op-by-op step", who);
    if (n == 1) return ifa_fail(IFA_ERR_STATE, "%s: one row is not a batched step (ifa_model_decode / ifa_model_decode_sampled feed a single row on the device)", who);
    {
        BatchRoute R;
        int rc = batch_route_of_call(m, n, R);
        if (rc) return rc;
        if (R.chunk) return ifa_fail(IFA_ERR_STATE, "%s: %d rows run as steps of %d; the device-fed steps take what ONE fused step takes", who, n, R.chunk);
        if (R.kind != BATCH_FUSED) return ifa_fail(IFA_ERR_STATE, "%s: the batched step of this model runs op by op, not as the fused step", who);
        if (!R.captured) return ifa_fail(IFA_ERR_STATE, "%s: the fused batched step is not captured (option graph = 0)", who);
    }
    IFA_REQUIRE(n <= IFA_BATCH_ROWS_MAX, "%s: n %d above %d", who, n, IFA_BATCH_ROWS_MAX);
    // ---- arguments
    const ifa_model_config &c = m->cfg;
    const size_t V = m->g[T_LM_HEAD].rows;
    const int n_slots = m->slots.empty() ? 1 : (int)m->slots.size();
    for (int r = 0; r < n; r++) {
        IFA_REQUIRE(positions_host[r] >= 0 && positions_host[r] + n_steps <= c.max_ctx, "%s: row %d: position %d + %d steps outside max_ctx %d", who, r, positions_host[r], n_steps, c.max_ctx);
        IFA_REQUIRE(kv_slots_host[r] >= 0 && kv_slots_host[r] < n_slots, "%s: row %d: KV slot %d of %d", who, r, kv_slots_host[r], n_slots);
        for (int r2 = 0; r2 < r; r2++) IFA_REQUIRE(kv_slots_host[r2] != kv_slots_host[r], "%s: KV slot %d used twice", who, kv_slots_host[r]);
        IFA_REQUIRE(tokens_host[r] >= 0 && (size_t)tokens_host[r] < V, "%s: row %d: token %d outside the vocabulary", who, r, tokens_host[r]);
        if (!rows) continue;
        const ifa_batch_row &b = rows[r];
        IFA_REQUIRE(b.struct_size == (int)sizeof(ifa_batch_row), "%s: row %d: struct_size is not %zu", who, r, sizeof(ifa_batch_row));
        IFA_REQUIRE(ifa_sr::sr_strategy_ok(b.p.strategy_id), "%s: row %d: strategy %d is not one of 1 sample.std, 2 greedy, 3 top_k, 4 sample.top_p, 7 min_p", who, r, b.p.strategy_id);
        IFA_REQUIRE(b.p.pool_size >= 1 && b.p.pool_size <= IFA_POOL_MAX, "%s: row %d: pool_size %d outside 1..%d", who, r, b.p.pool_size, IFA_POOL_MAX);
        IFA_REQUIRE(b.n_stop >= 0 && b.n_stop <= IFA_BATCH_STOP_MAX, "%s: row %d: n_stop %d outside 0..%d", who, r, b.n_stop, IFA_BATCH_STOP_MAX);
        IFA_REQUIRE(b.state_slot >= -1 && (b.state_slot < 0 || (size_t)b.state_slot < m->la_slots), "%s: row %d: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, r, b.state_slot);
    }
    IFA_HIP_CHECK(hipSetDevice(c.device));
    hipStream_t s = m->stream;
    int rc;
    if (!m->bs_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(s));
        if ((rc = m->bs_blk.reserve(BS_WORDS))) return rc;
    }
    // ---- the rows that need a pool, the step's one pool length
    std::vector<int> rows_sel, adj;
    int k = 1;
    bool counting = false;
    for (int r = 0; rows && r < n; r++)
        if (row_pooled(rows[r])) {
            rows_sel.push_back(r); adj.push_back(rows[r].state_slot);
            k = std::max(k, rows[r].p.pool_size);
            counting = counting || rows[r].state_slot >= 0;
        }
    const int n_sel = (int)rows_sel.size();
    PoolFedGuard guard{m};
    if (n_sel && (rc = pool_fed_begin(m, k, n_sel, rows_sel.data(), adj.data(), who))) return rc;
    // ---- the call's values into device memory
    int *pin = m->bs_blk.pin, *dev = m->bs_blk.dev;
    memset(pin, 0, sizeof(int) * (size_t)BS_RING);
    memset(pin + BS_PARAMS, 0, sizeof(int) * (size_t)(BS_WORDS - BS_PARAMS));
    ifa_batch_feed_row *fr = (ifa_batch_feed_row *)(pin + BS_ROWS);
    ifa_sample_params *pp = (ifa_sample_params *)(pin + BS_PARAMS);
    unsigned long long *prng = (unsigned long long *)(pin + BS_RNG);
    for (int r = 0, j = 0; r < n; r++) {
        fr[r].live = 1; fr[r].kind = IFA_BATCH_KIND_ARGMAX; fr[r].state_slot = -1; fr[r].sel = -1;
        if (!rows) continue;
        const ifa_batch_row &b = rows[r];
        fr[r].n_stop = b.n_stop;
        memcpy(fr[r].stop_ids, b.stop_ids, sizeof(int) * (size_t)b.n_stop);
        fr[r].state_slot = b.state_slot;
        fr[r].rng_final = b.rng_state;
        if (!row_pooled(b)) continue;
        fr[r].kind = IFA_BATCH_KIND_DRAWN; fr[r].sel = j;
        pp[j] = b.p; prng[j] = b.rng_state; pin[BS_POOL_LEN + j] = b.p.pool_size;
        j++;
    }
    IFA_HIP_CHECK(hipMemcpyAsync(dev, pin, sizeof(int) * (size_t)BS_RING, hipMemcpyHostToDevice, s));
    IFA_HIP_CHECK(hipMemcpyAsync(dev + BS_PARAMS, pin + BS_PARAMS, sizeof(int) * (size_t)(BS_WORDS - BS_PARAMS), hipMemcpyHostToDevice, s));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } evg{e0, e1};
    if (elapsed_ms) { IFA_HIP_CHECK(hipEventCreate(&e0)); IFA_HIP_CHECK(hipEventCreate(&e1)); IFA_HIP_CHECK(hipEventRecord(e0, s)); }
    // ---- the steps
    ifa_batch_feed_args fa;
    memset(&fa, 0, sizeof(fa));
    for (int i = 0; i < n_steps; i++) {
        if ((rc = forward_batch(m, n, tokens_host, positions_host, kv_slots_host, nullptr, nullptr, false, i == 0 ? FED_FIRST : FED_NEXT))) return rc;
        if (i == 0) {      // (the first step has made sure of the tables)
            AttnRowH *rows_d = (AttnRowH *)m->batch_tab.dev.get();
            int *pos_d = (int *)(rows_d + m->layers.size() * (size_t)n);
            fa.struct_size = (int)sizeof(fa); fa.n = n; fa.layers = (int)m->layers.size(); fa.ring_steps = n_steps; fa.k_stride = 0;
            fa.rows = (ifa_batch_feed_row *)(dev + BS_ROWS); fa.step = dev + BS_STEP; fa.argmax = m->state + 8;
            fa.drawn = n_sel ? dev + BS_DRAWN : nullptr; fa.rng = n_sel ? (const unsigned long long *)(dev + BS_RNG) : nullptr;
            fa.tok = pos_d + n; fa.pos = pos_d; fa.attn_rows = rows_d; fa.ring = dev + BS_RING;
            fa.pair_slot = dev + BS_PAIR_SLOT; fa.pair_tok = dev + BS_PAIR_TOK; fa.err = dev + BS_ERR;
        }
        if (n_sel) {
            if ((rc = pool_fed_enqueue(m, m->logits))) return rc;
            int *counts, *ids; void *vals;
            pool_fed_block(m, &counts, &ids, &vals);
            if ((rc = ifa_batch_clamp_counts(counts, dev + BS_POOL_LEN, (size_t)n_sel, (ifa_stream)s))) return rc;
            if ((rc = ifa::sample_pool_launch(counts, ids, vals, (size_t)n_sel, k, (const ifa_sample_params *)(dev + BS_PARAMS), (unsigned long long *)(dev + BS_RNG),
                                              dev + BS_DRAWN, dev + BS_INDEX, nullptr, dev + BS_DRAW_ERR, nullptr, 1, s))) return rc;
        }
        if ((rc = ifa_batch_feed_rows(&fa, (ifa_stream)s))) return rc;
        // the emitted tokens are counted before the next step's processors read the slots
        if (counting && (rc = ifa_logit_state_add(dev + BS_PAIR_SLOT, dev + BS_PAIR_TOK, (size_t)n, V, m->la_slots, m->la_state, (ifa_stream)s))) return rc;
    }
    if (elapsed_ms) IFA_HIP_CHECK(hipEventRecord(e1, s));
    IFA_HIP_CHECK(hipMemcpyAsync(pin, dev, sizeof(int) * ((size_t)BS_RING + (size_t)n_steps * (size_t)n), hipMemcpyDeviceToHost, s));
    IFA_HIP_CHECK(hipStreamSynchronize(s));
    if ((rc = wait_err_check("device-fed batched steps"))) { drop_graphs(m); return rc; }      // (as the one-step entry: re-captured without the K-parts launches)
    if (pin[BS_ERR] != 0) {
        const int code = pin[BS_ERR] - 1;
        return ifa_fail(IFA_ERR_STATE, "%s: step %d, row %d had no token to draw (an empty candidate pool); the results of this call are not valid", who, code / n, code % n);
    }
    if (elapsed_ms) IFA_HIP_CHECK(hipEventElapsedTime(elapsed_ms, e0, e1));
    memcpy(out_tokens_host, pin + BS_RING, sizeof(int) * (size_t)n_steps * (size_t)n);
    for (int r = 0; r < n; r++) {
        emitted_host[r] = fr[r].emitted;
        if (rows) rows[r].rng_state = fr[r].rng_final;
    }
    return IFA_OK;
}

} // extern "C"
