// ifa_engine_batch_steps.hip -- ifa_model_decode_batch_steps: n_steps batched decode steps of the same n rows with one
// synchronisation.  The tables of the first step -- token, position and per layer (K cache, V cache, context) of every row -- go to
// the device once; every step then is
//   replay of the batched step captured WITHOUT its table upload and copy back (forward_batch with a TAIL_FED tail: the same body, so
//     the launches are those of ifa_model_decode_batch)
//   -> [logit processors of the pooled rows' state slots -> candidate pools (pool_rows_launch over the runs of a pool tail) -> clamp of the counts to
//      each row's own pool length -> draw (k_sample_pool)]                                       (only with a row that is not plainly greedy)
//   -> feed (csrc/ifa_batch_feed.hip): token per row, stop ids, ring, token / position / context of every live row + 1
//   -> [one more occurrence of every emitted token in its row's state slot]
// all plain launches on the worker's stream behind the replay.  The pooled rows and their state slots are the same for every step of
// the call, so they go to the device once, and their runs (ifa_pool_rows_plan.h) are planned once.  What differs from call to call lives in
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

static bool row_pooled(const ifa_batch_row &r) { return r.p.strategy_id != ifa_sr::SR_GREEDY || r.state_slot >= 0; }

} // namespace ifae

extern "C" {

int ifa_model_batch_steps_rows(ifa_model *m)
{
    using namespace ifae;
    if (!m || !m->finalized || device_tail_refusal(m, true, true)) return 0;
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
    int rc = device_tail_refusals(m, who, true, true, "the device-fed steps take the fused, captured step of a single-device worker");
    if (rc) return rc;
    if (n == 1) return ifa_fail(IFA_ERR_STATE, "%s: one row is not a batched step (ifa_model_decode / ifa_model_decode_sampled feed a single row on the device)", who);
    {
        BatchRoute R;
        if ((rc = batch_route_of_call(m, n, R))) return rc;
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
    if (!m->bs_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(s));
        if ((rc = m->bs_blk.reserve(1))) return rc;
    }
    // ---- the rows that need a pool, the step's one pool length: pools of the call's own, never copied to the host
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
    std::vector<PoolRun> runs;
    int *slot_dev = nullptr;
    if (n_sel) {
        m->pool_adj_next.clear();      // (a pool call: whatever ifa_model_pool_adjust armed is consumed)
        const std::vector<int> slots = adj;
        if ((rc = pool_ready(m, k, n_sel, adj, who))) return rc;
        int *slot_pin = m->pool_idx.pin + pool_idx_rows(m);
        slot_dev = m->pool_idx.dev + pool_idx_rows(m);
        for (int j = 0; j < n_sel; j++) { m->pool_idx.pin[j] = rows_sel[j]; slot_pin[j] = std::max(slots[j], 0); }
        hipError_t e = hipMemcpyAsync(m->pool_idx.dev, m->pool_idx.pin, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(slot_dev, slot_pin, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return ifa_fail(IFA_ERR_HIP, "%s: upload of the pooled rows failed: %s", who, hipGetErrorString(e));
        (void)pool_rows_plan(rows_sel.data(), adj.empty() ? nullptr : adj.data(), n_sel, 0, 0, n, runs);      // one chunk, cursor 0
    }
    const PoolBlock B = pool_block(m->pool_blk.dev.get(), n_sel, k, false);      // (no step of the call hands a log-sum-exp to anybody)
    // ---- the call's values into device memory: [rows, ring) and [params, end) -- the ring is the device's
    BatchStepsBlk *pin = m->bs_blk.pin, *dev = m->bs_blk.dev;
    constexpr size_t ring_off = offsetof(BatchStepsBlk, ring), params_off = offsetof(BatchStepsBlk, params);
    memset(pin, 0, ring_off);
    memset((char *)pin + params_off, 0, sizeof(BatchStepsBlk) - params_off);
    ifa_batch_feed_row *fr = pin->rows;
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
        pin->params[j] = b.p; pin->rng[j] = b.rng_state; pin->pool_len[j] = b.p.pool_size;
        j++;
    }
    IFA_HIP_CHECK(hipMemcpyAsync(dev, pin, ring_off, hipMemcpyHostToDevice, s));
    IFA_HIP_CHECK(hipMemcpyAsync((char *)dev + params_off, (const char *)pin + params_off, sizeof(BatchStepsBlk) - params_off, hipMemcpyHostToDevice, s));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } evg{e0, e1};
    if (elapsed_ms) { IFA_HIP_CHECK(hipEventCreate(&e0)); IFA_HIP_CHECK(hipEventCreate(&e1)); IFA_HIP_CHECK(hipEventRecord(e0, s)); }
    // ---- the steps
    ifa_batch_feed_args fa;
    memset(&fa, 0, sizeof(fa));
    StepTail fed; TailCursor cur;
    fed.kind = TAIL_FED;
    for (int i = 0; i < n_steps; i++) {
        fed.fed_first = i == 0;
        if ((rc = forward_batch(m, n, tokens_host, positions_host, kv_slots_host, nullptr, nullptr, fed, cur))) return rc;
        if (i == 0) {      // (the first step has made sure of the tables)
            AttnRowH *rows_d = (AttnRowH *)m->batch_tab.dev.get();
            int *pos_d = (int *)(rows_d + m->layers.size() * (size_t)n);
            fa.struct_size = (int)sizeof(fa); fa.n = n; fa.layers = (int)m->layers.size(); fa.ring_steps = n_steps; fa.k_stride = 0;
            fa.rows = dev->rows; fa.step = &dev->step; fa.argmax = m->state + 8;
            fa.drawn = n_sel ? dev->drawn : nullptr; fa.rng = n_sel ? dev->rng : nullptr;
            fa.tok = pos_d + n; fa.pos = pos_d; fa.attn_rows = rows_d; fa.ring = dev->ring;
            fa.pair_slot = dev->pair_slot; fa.pair_tok = dev->pair_tok; fa.err = &dev->err;
        }
        if (n_sel) {
            for (const PoolRun &r : runs)
                if ((rc = pool_rows_launch(m, B, k, m->logits, m->pool_idx.dev + r.ja, r.armed ? slot_dev + r.ja : nullptr, r.ja, r.jb))) return rc;
            if ((rc = ifa_batch_clamp_counts(B.counts, dev->pool_len, (size_t)n_sel, (ifa_stream)s))) return rc;
            if ((rc = ifa::sample_pool_launch(B.counts, B.ids, B.vals, (size_t)n_sel, k, dev->params, dev->rng, dev->drawn, dev->index, nullptr, &dev->draw_err, nullptr, 1, s))) return rc;
        }
        if ((rc = ifa_batch_feed_rows(&fa, (ifa_stream)s))) return rc;
        // the emitted tokens are counted before the next step's processors read the slots
        if (counting && (rc = ifa_logit_state_add(dev->pair_slot, dev->pair_tok, (size_t)n, V, m->la_slots, m->la_state, (ifa_stream)s))) return rc;
    }
    if (elapsed_ms) IFA_HIP_CHECK(hipEventRecord(e1, s));
    IFA_HIP_CHECK(hipMemcpyAsync(pin, dev, ring_off + sizeof(int) * (size_t)n_steps * (size_t)n, hipMemcpyDeviceToHost, s));
    IFA_HIP_CHECK(hipStreamSynchronize(s));
    if ((rc = wait_err_check("device-fed batched steps"))) { drop_graphs(m); return rc; }      // (as the one-step entry: re-captured without the K-parts launches)
    if (pin->err != 0) {
        const int code = pin->err - 1;
        return ifa_fail(IFA_ERR_STATE, "%s: step %d, row %d had no token to draw (an empty candidate pool); the results of this call are not valid", who, code / n, code % n);
    }
    if (elapsed_ms) IFA_HIP_CHECK(hipEventElapsedTime(elapsed_ms, e0, e1));
    memcpy(out_tokens_host, pin->ring, sizeof(int) * (size_t)n_steps * (size_t)n);
    for (int r = 0; r < n; r++) {
        emitted_host[r] = fr[r].emitted;
        if (rows) rows[r].rng_state = fr[r].rng_final;
    }
    return IFA_OK;
}

} // extern "C"
