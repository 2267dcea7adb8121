// ifa_engine_pool.hip -- the tails of the worker's steps (StepTail, ifa_engine_state.h; DESIGN.md "Step tails") and the entry points
// that end in a candidate pool (ifa_model_decode_pool / _decode_batch_pool / _forward_pool).  An entry point builds its tail, runs the
// ordinary step -- whatever route decode_impl / decode_batch_impl / forward_impl takes for this model -- and that step calls
// tail_enqueue() on its logits in front of its one stream synchronisation.  A pool tail is one more launch (csrc/ifa_topk_pool.hip)
// and one copy of (counts, ids, values) into pinned staging; nothing is captured: the launches follow the graph replay on the stream.
// Logit processors (ifa_logit_adjust.hip): rows armed by ifa_model_pool_adjust pass through ifa_logit_adjust_rows into m->la_adj first
// and the pool / log-sum-exp launches read those rows.  pool_rows_launch is the one place that enqueues this sequence: the sampled,
// draft-verify and device-fed tails call it too and differ in what follows it.
#include <algorithm>
#include <cmath>
#include "ifa_engine_state.h"

namespace ifa {
int topk_pool_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, int k, const unsigned *excl,
                   int *ids_out, void *vals_out, int *count_out, hipStream_t s);
int lse_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, const int *targets_dev, float *lse_out,
             float *target_out, float *part_dev, hipStream_t s);
int logit_adjust_rows(const void *logits, size_t row_stride, const int *row_idx_dev, const int *state_slot_dev, size_t rows, size_t n,
                      const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out, hipStream_t s);
}

namespace ifae {

// state / bias / params for every KV slot the worker has now (first use, or more slots since: the old rows are kept)
static int logit_state_reserve(ifa_model *m)
{
    const size_t V = m->g[T_LM_HEAD].rows, want = std::max<size_t>(m->slots.size(), 1);
    if (want <= m->la_slots) return IFA_OK;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    DevBuf<unsigned> st; DevBuf<float> bs, pr;
    if (st.alloc(want * V) || bs.alloc(want * V) || pr.alloc(want * 3))
        return ifa_fail(IFA_ERR_NOMEM, "logit processors: no memory for the state of %zu slots x %zu ids", want, V);
    // a slot nobody has reset yet reads as neutral: no counts, no bias, {1, 0, 0}
    std::vector<float> neutral(want * 3, 0.0f);
    for (size_t i = 0; i < want; i++) neutral[i * 3] = 1.0f;
    hipError_t e = hipMemset(st, 0, want * V * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(bs, 0, want * V * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(pr, neutral.data(), want * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && m->la_slots) {
        e = hipMemcpy(st, m->la_state, m->la_slots * V * sizeof(unsigned), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(bs, m->la_bias, m->la_slots * V * sizeof(float), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(pr, m->la_params, m->la_slots * 3 * sizeof(float), hipMemcpyDeviceToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return ifa_fail(IFA_ERR_HIP, "logit processors: state setup failed: %s", hipGetErrorString(e));
    m->la_state = std::move(st); m->la_bias = std::move(bs); m->la_params = std::move(pr); m->la_slots = want;
    return IFA_OK;
}

const char *device_tail_refusal(const ifa_model *m, bool needs_embd, bool fused_only)
{
    if (m->cfg.tp_size > 1 || m->topo) return "the vocabulary of a partitioned worker is sharded";
    if (!m->g[T_LM_HEAD].present() || (needs_embd && !m->g[T_EMBD].present())) return needs_embd ? "embeddings / lm_head missing (pipeline stage worker)" : "lm_head missing (pipeline stage worker)";
    if (fused_only && m->opt_exact_order) return "option exact_order steps row by row on the host";
    if (fused_only && m->opt_perf_stat) return "option perf_stat times the op-by-op step";
    return nullptr;
}

int device_tail_refusals(const ifa_model *m, const char *who, bool needs_embd, bool fused_only, const char *hint)
{
    const char *why = device_tail_refusal(m, needs_embd, fused_only);
    return why ? ifa_fail(IFA_ERR_STATE, "%s: %s; %s", who, why, hint) : IFA_OK;
}

// staging for n_sel rows of k entries (grown on demand, outside any capture; one allocation serves every later step)
int pool_reserve(ifa_model *m, int n_sel, int k)
{
    const size_t bytes = pool_block(nullptr, std::max(n_sel, 8), IFA_POOL_MAX >= k ? IFA_POOL_MAX : k, true).bytes;
    int rc;
    if (bytes > m->pool_blk.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->pool_blk.reserve(bytes))) return rc;
    }
    if ((size_t)n_sel > pool_idx_rows(m)) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        // row indices [cap] | state slots of armed rows [cap] (logit processors)
        if ((rc = m->pool_idx.reserve(2 * (size_t)std::max(n_sel, 64)))) return rc;
    }
    return IFA_OK;
}

int la_adj_reserve(ifa_model *m, size_t rows, const char *who)
{
    const size_t V = m->g[T_LM_HEAD].rows, want = std::max<size_t>(rows, 8);
    if (want * V <= m->la_adj.cap()) return IFA_OK;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->la_adj.alloc(want * V)) return ifa_fail(IFA_ERR_NOMEM, "%s: no memory for %zu adjusted rows", who, want);
    return IFA_OK;
}

int pool_rows_launch(ifa_model *m, const PoolBlock &B, int k, const half_t *logits, const int *idx, const int *slots, int ja, int jb)
{
    const size_t V = m->g[T_LM_HEAD].rows, rows = (size_t)(jb - ja);
    int rc = IFA_OK;
    const void *src = logits;
    if (slots) {
        half_t *adj = m->la_adj + (size_t)ja * V;
        if ((rc = logit_adjust_rows(logits, V, idx, slots, rows, V, m->la_state, m->la_bias, m->la_params, adj, m->stream))) return rc;
        src = adj; idx = nullptr;
    }
    if ((rc = topk_pool_rows(src, V, idx, rows, V, k, m->pool_excl, B.ids + (size_t)ja * k, B.vals + (size_t)ja * k, B.counts + ja, m->stream))) return rc;
    if (B.lse && (rc = lse_rows(src, V, idx, rows, V, nullptr, B.lse + ja, nullptr, m->lse_part, m->stream))) return rc;
    return IFA_OK;
}

// TAIL_POOL: the pooled rows this step serves, then -- behind the call's last step -- the copy of the block
static int pool_enqueue(ifa_model *m, const StepTail &t, TailCursor &cur, const half_t *logits, int n_rows)
{
    const size_t V = m->g[T_LM_HEAD].rows;
    const int n_sel = t.n;
    const bool adj = t.adj != nullptr;
    const PoolBlock B = pool_block(m->pool_blk.dev.get(), n_sel, t.k, t.lse);
    int *slot_pin = m->pool_idx.pin + pool_idx_rows(m), *slot_dev = m->pool_idx.dev + pool_idx_rows(m);
    int rc = IFA_OK;
    if (!t.rows_sel) {                 // a single-query step: its last row
        if (adj) {
            slot_pin[0] = t.adj[0];
            IFA_HIP_CHECK(hipMemcpyAsync(slot_dev, slot_pin, sizeof(int), hipMemcpyHostToDevice, m->stream));
        }
        if ((rc = pool_rows_launch(m, B, t.k, logits + (size_t)(n_rows - 1) * V, nullptr, adj ? slot_dev : nullptr, 0, 1))) return rc;
        cur.done = 1;
    } else {                           // a batched step (or one chunk of it): the wanted rows among [chunk0, chunk0 + n_rows)
        std::vector<PoolRun> runs;
        const int j0 = cur.done, j1 = pool_rows_plan(t.rows_sel, t.adj, n_sel, j0, cur.chunk0, n_rows, runs);
        if (j1 > j0) {
            for (int j = j0; j < j1; j++) m->pool_idx.pin[j] = t.rows_sel[j] - cur.chunk0;
            IFA_HIP_CHECK(hipMemcpyAsync(m->pool_idx.dev + j0, m->pool_idx.pin + j0, sizeof(int) * (size_t)(j1 - j0), hipMemcpyHostToDevice, m->stream));
            if (adj) {
                for (int j = j0; j < j1; j++) slot_pin[j] = std::max(t.adj[j], 0);
                IFA_HIP_CHECK(hipMemcpyAsync(slot_dev + j0, slot_pin + j0, sizeof(int) * (size_t)(j1 - j0), hipMemcpyHostToDevice, m->stream));
            }
            for (const PoolRun &r : runs)      // each run its own launches (nothing or everything armed, the usual case: one run)
                if ((rc = pool_rows_launch(m, B, t.k, logits, m->pool_idx.dev + r.ja, r.armed ? slot_dev + r.ja : nullptr, r.ja, r.jb))) return rc;
        }
        cur.done = j1;
        if (!cur.last_chunk) return IFA_OK;
    }
    IFA_HIP_CHECK(hipMemcpyAsync(m->pool_blk.pin, m->pool_blk.dev, B.bytes, hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

int tail_enqueue(ifa_model *m, const StepTail &t, TailCursor &cur, const half_t *logits, int n_rows)
{
    switch (t.kind) {
    case TAIL_POOL: return pool_enqueue(m, t, cur, logits, n_rows);
    case TAIL_SCORE: return score_enqueue(m, t, cur, logits, n_rows);
    case TAIL_DRAFT_VERIFY: return draft_sampled_enqueue(m, t, logits, n_rows);
    case TAIL_NONE: case TAIL_SAMPLED: case TAIL_FED: break;      // (the draw is inside the step; a fed step's caller enqueues what follows)
    }
    return IFA_OK;
}

int pool_ready(ifa_model *m, int k, int n_sel, std::vector<int> &adj, const char *who)
{
    if (std::all_of(adj.begin(), adj.end(), [](int slot) { return slot < 0; })) adj.clear();
    IFA_REQUIRE(adj.empty() || (int)adj.size() == n_sel, "%s: ifa_model_pool_adjust armed %zu rows, the step pools %d", who, adj.size(), n_sel);
    IFA_REQUIRE(k >= 1 && k <= IFA_POOL_MAX, "%s: k %d outside 1..%d", who, k, IFA_POOL_MAX);
    int rc = device_tail_refusals(m, who, false, false, "the pool is built on the host there");
    if (rc) return rc;
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    if ((rc = pool_reserve(m, n_sel, k))) return rc;
    if (m->opt_pool_lse && (rc = lse_part_reserve(m))) return rc;
    m->pool_lse_last.clear();
    for (int slot : adj)
        if (slot >= 0 && (size_t)slot >= m->la_slots) return ifa_fail(IFA_ERR_STATE, "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, slot);
    if (!adj.empty() && (rc = la_adj_reserve(m, (size_t)n_sel, who))) return rc;
    return IFA_OK;
}

// A pool entry point: what ifa_model_pool_adjust armed belongs to THIS call -- moved out at entry, whether the call gets as far as a
// launch or not, the argument checks in front of ready() included.  The tail points into the call's own array.
struct PoolCall {
    StepTail t; TailCursor cur; std::vector<int> adj;
    explicit PoolCall(ifa_model *m) { if (m) adj.swap(m->pool_adj_next); }
    int ready(ifa_model *m, int k, int n_sel, const int *rows_sel, const char *who)
    {
        const int rc = pool_ready(m, k, n_sel, adj, who);
        if (rc) return rc;
        t.kind = TAIL_POOL; t.k = k; t.n = n_sel; t.rows_sel = rows_sel;
        t.lse = m->opt_pool_lse != 0;
        t.adj = adj.empty() ? nullptr : adj.data();
        return IFA_OK;
    }
};

// after the step: copies the staged block out if the step succeeded and every wanted row was served
static int pool_finish(ifa_model *m, const PoolCall &c, int step_rc, int *ids_host, unsigned short *vals_host, int *counts_host, const char *who)
{
    const StepTail &t = c.t;
    if (step_rc) return step_rc;
    if (c.cur.done != t.n) return ifa_fail(IFA_ERR_STATE, "%s: the step served %d of %d pools", who, c.cur.done, t.n);
    const PoolBlock B = pool_block(m->pool_blk.pin.get(), t.n, t.k, t.lse);
    if (B.lse) m->pool_lse_last.assign(B.lse, B.lse + t.n);
    memcpy(counts_host, B.counts, sizeof(int) * (size_t)t.n);
    memcpy(ids_host, B.ids, sizeof(int) * (size_t)t.n * t.k);
    memcpy(vals_host, B.vals, sizeof(uint16_t) * (size_t)t.n * t.k);
    return IFA_OK;
}

} // namespace ifae

extern "C" {

int ifa_model_set_pool_excluded(ifa_model *m, const int *ids_host, int n)
{
    IFA_REQUIRE(m && m->finalized, "ifa_model_set_pool_excluded: model not finalized");
    IFA_REQUIRE(n >= 0 && (n == 0 || ids_host), "ifa_model_set_pool_excluded: bad arguments");
    IFA_REQUIRE(m->g[T_LM_HEAD].present(), "ifa_model_set_pool_excluded: lm_head missing");
    const size_t V = m->g[T_LM_HEAD].rows, words = (V + 31) / 32;
    for (int i = 0; i < n; i++) IFA_REQUIRE(ids_host[i] >= 0 && (size_t)ids_host[i] < V, "ifa_model_set_pool_excluded: id %d outside the vocabulary", ids_host[i]);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (n == 0) { m->pool_excl.reset(); return IFA_OK; }
    std::vector<unsigned> bits(words, 0u);
    for (int i = 0; i < n; i++) bits[(size_t)ids_host[i] >> 5] |= 1u << (ids_host[i] & 31);
    if (!m->pool_excl) { int rc = m->pool_excl.alloc(words); if (rc) return rc; }
    IFA_HIP_CHECK(hipMemcpy(m->pool_excl, bits.data(), words * sizeof(unsigned), hipMemcpyHostToDevice));
    return IFA_OK;
}

int ifa_model_logit_state_reset(ifa_model *m, int kv_slot, const int *prompt_host, int n_prompt, float rep, float freq, float pres,
                                const int *bias_ids_host, const float *bias_vals_host, int n_bias)
{
    const char *who = "ifa_model_logit_state_reset";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    int rc = device_tail_refusals(m, who, false, false, "logit processors run on a single-device worker");
    if (rc) return rc;
    const size_t V = m->g[T_LM_HEAD].rows;
    IFA_REQUIRE(kv_slot >= 0 && (size_t)kv_slot < std::max<size_t>(m->slots.size(), 1), "%s: KV slot %d (the worker has %zu)", who, kv_slot, std::max<size_t>(m->slots.size(), 1));
    IFA_REQUIRE(n_prompt >= 0 && n_prompt <= m->cfg.max_ctx && (n_prompt == 0 || prompt_host), "%s: %d prompt tokens", who, n_prompt);
    IFA_REQUIRE(std::isfinite(rep) && rep > 0.0f, "%s: repetition penalty %g must be finite and above 0", who, (double)rep);
    IFA_REQUIRE(std::isfinite(freq) && std::isfinite(pres), "%s: frequency penalty %g / presence penalty %g must be finite", who, (double)freq, (double)pres);
    IFA_REQUIRE(n_bias >= 0 && n_bias <= IFA_LOGIT_BIAS_MAX && (n_bias == 0 || (bias_ids_host && bias_vals_host)), "%s: %d logit_bias entries (at most %d)", who, n_bias, IFA_LOGIT_BIAS_MAX);
    for (int i = 0; i < n_prompt; i++) IFA_REQUIRE(prompt_host[i] >= 0 && (size_t)prompt_host[i] < V, "%s: prompt id %d outside the vocabulary", who, prompt_host[i]);
    {
        std::vector<int> seen(bias_ids_host, bias_ids_host + n_bias);
        std::sort(seen.begin(), seen.end());
        for (int i = 0; i < n_bias; i++) {
            IFA_REQUIRE(seen[(size_t)i] >= 0 && (size_t)seen[(size_t)i] < V, "%s: logit_bias id %d outside the vocabulary", who, seen[(size_t)i]);
            IFA_REQUIRE(i == 0 || seen[(size_t)i] != seen[(size_t)i - 1], "%s: logit_bias id %d given twice", who, seen[(size_t)i]);
            IFA_REQUIRE(std::isfinite(bias_vals_host[i]) || bias_vals_host[i] == -INFINITY, "%s: logit_bias value %g must be finite or -inf", who, (double)bias_vals_host[i]);
        }
    }
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    if ((rc = logit_state_reserve(m))) return rc;
    // staging: prompt [n_prompt] | bias ids [n_bias] | bias values [n_bias]
    const size_t need = (size_t)n_prompt + 2 * (size_t)n_bias;
    if (need > m->la_reset.cap()) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if ((rc = m->la_reset.reserve(std::max<size_t>(need, (size_t)m->cfg.max_ctx + 2 * IFA_LOGIT_BIAS_MAX)))) return rc;
    }
    int *pin = m->la_reset.pin, *dev = m->la_reset.dev;
    if (n_prompt) memcpy(pin, prompt_host, sizeof(int) * (size_t)n_prompt);
    if (n_bias) {
        memcpy(pin + n_prompt, bias_ids_host, sizeof(int) * (size_t)n_bias);
        memcpy(pin + n_prompt + n_bias, bias_vals_host, sizeof(float) * (size_t)n_bias);
    }
    if (need) IFA_HIP_CHECK(hipMemcpyAsync(dev, pin, need * sizeof(int), hipMemcpyHostToDevice, m->stream));
    rc = ifa_logit_state_reset(kv_slot, dev, (size_t)n_prompt, rep, freq, pres, dev + n_prompt, (const float *)(dev + n_prompt + n_bias),
                               (size_t)n_bias, V, m->la_state, m->la_bias, m->la_params, (ifa_stream)m->stream);
    if (rc) return rc;
    IFA_HIP_CHECK(hipStreamSynchronize(m->stream));      // (the staging block is free again; a query starts once)
    return IFA_OK;
}

int ifa_model_logit_state_add(ifa_model *m, int n, const int *kv_slots_host, const int *tokens_host)
{
    const char *who = "ifa_model_logit_state_add";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    int rc = device_tail_refusals(m, who, false, false, "logit processors run on a single-device worker");
    if (rc) return rc;
    IFA_REQUIRE(n >= 0 && n <= ifa_model::RING && (n == 0 || (kv_slots_host && tokens_host)), "%s: %d pairs (at most %d)", who, n, ifa_model::RING);
    if (n == 0) return IFA_OK;
    if (!m->la_state) return ifa_fail(IFA_ERR_STATE, "%s: no logit state yet (ifa_model_logit_state_reset first)", who);
    const size_t V = m->g[T_LM_HEAD].rows;
    for (int i = 0; i < n; i++)
        IFA_REQUIRE(kv_slots_host[i] >= 0 && (size_t)kv_slots_host[i] < m->la_slots && tokens_host[i] >= 0 && (size_t)tokens_host[i] < V,
                    "%s: pair %d = (slot %d, token %d) outside %zu slots x %zu ids", who, i, kv_slots_host[i], tokens_host[i], m->la_slots, V);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    constexpr size_t BLOCK = 2 * (size_t)ifa_model::RING;
    for (int i = 0; i < ifa_model::LA_RING; i++) if (!m->la_ev[i]) IFA_HIP_CHECK(hipEventCreateWithFlags(&m->la_ev[i].e, hipEventDisableTiming));
    if ((rc = m->la_ring.reserve(ifa_model::LA_RING * BLOCK))) return rc;
    const int b = (int)(m->la_calls++ % ifa_model::LA_RING);
    if (m->la_ev_used[b]) IFA_HIP_CHECK(hipEventSynchronize(m->la_ev[b]));      // (done long ago unless LA_RING calls are in flight)
    int *pin = m->la_ring.pin + (size_t)b * BLOCK, *dev = m->la_ring.dev + (size_t)b * BLOCK;
    memcpy(pin, kv_slots_host, sizeof(int) * (size_t)n);
    memcpy(pin + n, tokens_host, sizeof(int) * (size_t)n);
    IFA_HIP_CHECK(hipMemcpyAsync(dev, pin, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, m->stream));
    if ((rc = ifa_logit_state_add(dev, dev + n, (size_t)n, V, m->la_slots, m->la_state, (ifa_stream)m->stream))) return rc;
    IFA_HIP_CHECK(hipEventRecord(m->la_ev[b], m->stream));
    m->la_ev_used[b] = true;
    return IFA_OK;
}

int ifa_model_pool_adjust(ifa_model *m, int n_sel, const int *state_slots_host)
{
    const char *who = "ifa_model_pool_adjust";
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    m->pool_adj_next.clear();
    int rc = device_tail_refusals(m, who, false, false, "logit processors run on a single-device worker");
    if (rc) return rc;
    IFA_REQUIRE(n_sel >= 0 && n_sel <= ifa_model::RING && (n_sel == 0 || state_slots_host), "%s: n_sel %d", who, n_sel);
    for (int j = 0; j < n_sel; j++)
        IFA_REQUIRE(state_slots_host[j] >= -1 && (state_slots_host[j] < 0 || (size_t)state_slots_host[j] < m->la_slots),
                    "%s: row %d: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, j, state_slots_host[j]);
    m->pool_adj_next.assign(state_slots_host, state_slots_host + n_sel);
    return IFA_OK;
}

int ifa_model_pool_lse(ifa_model *m, float *lse_host, int cap, int *n_out)
{
    IFA_REQUIRE(m && n_out && cap >= 0 && (cap == 0 || lse_host), "ifa_model_pool_lse: bad arguments");
    const int n = (int)m->pool_lse_last.size();
    if (n > cap) return ifa_fail(IFA_ERR_ARG, "ifa_model_pool_lse: the last pool step staged %d values, room for %d", n, cap);
    if (n) memcpy(lse_host, m->pool_lse_last.data(), sizeof(float) * (size_t)n);
    *n_out = n;
    return IFA_OK;
}

int ifa_model_decode_pool(ifa_model *m, int token, int pos, int k, int *next_token_host,
                          int *pool_ids_host, unsigned short *pool_vals_host, int *pool_count_host)
{
    const char *who = "ifa_model_decode_pool";
    PoolCall c(m);
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(pool_ids_host && pool_vals_host && pool_count_host, "%s: null pointer", who);
    int rc = c.ready(m, k, 1, nullptr, who);
    if (rc) return rc;
    int next = -1;
    rc = decode_impl(m, token, pos, 1, &next, nullptr, false, c.t, c.cur);
    rc = pool_finish(m, c, rc, pool_ids_host, pool_vals_host, pool_count_host, who);
    if (!rc && next_token_host) *next_token_host = next;
    return rc;
}

int ifa_model_forward_pool(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev, int k,
                           int *next_token_host, int *pool_ids_host, unsigned short *pool_vals_host, int *pool_count_host)
{
    const char *who = "ifa_model_forward_pool";
    PoolCall c(m);
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(tokens_host && n_tokens >= 1 && pool_ids_host && pool_vals_host && pool_count_host, "%s: bad arguments", who);
    int rc = c.ready(m, k, 1, nullptr, who);
    if (rc) return rc;
    int next = -1;
    rc = forward_impl(m, tokens_host, n_tokens, prefix_len, logits_out_dev, &next, c.t, c.cur);
    // (option exact_order feeds a prompt row by row: every row's step stages its pool, the last one's is what remains)
    rc = pool_finish(m, c, rc, pool_ids_host, pool_vals_host, pool_count_host, who);
    if (!rc && next_token_host) *next_token_host = next;
    return rc;
}

int ifa_model_decode_batch_pool(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                                int *next_tokens_host, int k, const int *rows_sel_host, int n_sel,
                                int *pool_ids_host, unsigned short *pool_vals_host, int *pool_counts_host)
{
    const char *who = "ifa_model_decode_batch_pool";
    PoolCall c(m);
    IFA_REQUIRE(m && m->finalized, "%s: model not finalized", who);
    IFA_REQUIRE(n >= 1 && n_sel >= 0 && n_sel <= n, "%s: n %d n_sel %d", who, n, n_sel);
    if (n_sel == 0) return ifa_model_decode_batch(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, nullptr);
    IFA_REQUIRE(rows_sel_host && pool_ids_host && pool_vals_host && pool_counts_host, "%s: null pointer", who);
    for (int j = 0; j < n_sel; j++)
        IFA_REQUIRE(rows_sel_host[j] >= 0 && rows_sel_host[j] < n && (j == 0 || rows_sel_host[j] > rows_sel_host[j - 1]),
                    "%s: rows_sel must be strictly ascending indices below n = %d", who, n);
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "%s: option exact_order steps the rows one by one; take ifa_model_decode_pool per query", who);
    int rc = c.ready(m, k, n_sel, rows_sel_host, who);
    if (rc) return rc;
    rc = decode_batch_impl(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, nullptr, c.t, c.cur);
    return pool_finish(m, c, rc, pool_ids_host, pool_vals_host, pool_counts_host, who);
}

} // extern "C"
