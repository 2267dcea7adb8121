// ifa_engine_pool.hip -- worker steps that end in a candidate pool (ifa_model_decode_pool / _decode_batch_pool / _forward_pool):
// the entry point arms m->pool, runs the ordinary step -- whatever route ifa_model_decode / _decode_batch / _forward takes for
// this model -- and that step calls pool_enqueue() on its logits in front of its one stream synchronisation: one more launch
// (csrc/ifa_topk_pool.hip) and one copy of (counts, ids, values) into pinned staging.  Nothing is captured: the pool launch
// follows the graph replay on the stream.
// Logit processors (ifa_logit_adjust.hip) hook in here: rows armed by ifa_model_pool_adjust pass through ifa_logit_adjust_rows into
// m->la_adj first and the pool / log-sum-exp launches read those rows; with nothing armed the launches are the ones above.
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

// counts [n_sel] | (with_lse: lse [n_sel] |) ids [n_sel][k] | F16 bits [n_sel][k]
static size_t pool_block_bytes(int n_sel, int k, bool with_lse) { return (size_t)n_sel * (with_lse ? 8 : 4) + (size_t)n_sel * (size_t)k * 6; }

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

static int logit_partitioned(const ifa_model *m, const char *who)
{
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "%s: the vocabulary of a partitioned worker is sharded; logit processors run on a single-device worker", who);
    if (!m->g[T_LM_HEAD].present()) return ifa_fail(IFA_ERR_STATE, "%s: lm_head missing (pipeline stage worker)", who);
    return IFA_OK;
}

// rows the index block serves: its second half holds the state slots of the armed rows
static size_t pool_idx_rows(const ifa_model *m) { return m->pool_idx.cap() / 2; }

// staging for n_sel rows of k entries (grown on demand, outside any capture; one allocation serves every later step)
int pool_reserve(ifa_model *m, int n_sel, int k)
{
    const size_t bytes = pool_block_bytes(std::max(n_sel, 8), IFA_POOL_MAX >= k ? IFA_POOL_MAX : k, true);
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

// pool (+ lse) of pooled rows [ja, jb): armed rows first pass through the logit processors into la_adj rows [ja, jb) and are read
// from there; idx (null: the step's one row) indexes `logits`
static int pool_rows_launch(ifa_model *m, const half_t *logits, const int *idx, int ja, int jb, bool armed)
{
    ifa_model::PoolReq &R = m->pool;
    const size_t V = m->g[T_LM_HEAD].rows, rows = (size_t)(jb - ja);
    const int k = R.k, n_sel = R.n_sel;
    int *counts = (int *)m->pool_blk.dev.get();
    float *lse = R.lse ? (float *)(counts + n_sel) : nullptr;
    int *ids = counts + (R.lse ? 2 : 1) * n_sel;
    uint16_t *vals = (uint16_t *)(ids + (size_t)n_sel * k);
    int rc = IFA_OK;
    const void *src = logits;
    if (armed) {
        half_t *adj = m->la_adj + (size_t)ja * V;
        if ((rc = logit_adjust_rows(logits, V, idx, m->pool_idx.dev + pool_idx_rows(m) + ja, rows, V, m->la_state, m->la_bias, m->la_params, adj, m->stream))) return rc;
        src = adj; idx = nullptr;
    }
    if ((rc = topk_pool_rows(src, V, idx, rows, V, k, m->pool_excl, ids + (size_t)ja * k, vals + (size_t)ja * k, counts + ja, m->stream))) return rc;
    if (lse && (rc = lse_rows(src, V, idx, rows, V, nullptr, lse + ja, nullptr, m->lse_part, m->stream))) return rc;
    return IFA_OK;
}

int pool_enqueue(ifa_model *m, const half_t *logits, int n_rows)
{
    if (m->dsv.k > 0) return draft_sampled_enqueue(m, logits, n_rows);      // (ifa_model_decode_draft_sampled: its own tail, no pool copy)
    ifa_model::PoolReq &R = m->pool;
    if (R.k <= 0) return IFA_OK;
    const int k = R.k, n_sel = R.n_sel;
    const bool adj = !R.adj.empty();
    int *slot_pin = m->pool_idx.pin + pool_idx_rows(m), *slot_dev = m->pool_idx.dev + pool_idx_rows(m);
    int rc = IFA_OK;
    if (!R.rows_sel) {                 // a single-query step: its one row
        if (adj) {
            slot_pin[0] = R.adj[0];
            IFA_HIP_CHECK(hipMemcpyAsync(slot_dev, slot_pin, sizeof(int), hipMemcpyHostToDevice, m->stream));
        }
        if ((rc = pool_rows_launch(m, logits, nullptr, 0, 1, adj))) return rc;
        R.done = 1;
    } else {                           // a batched step (or one chunk of it): the wanted rows among [chunk0, chunk0 + n_rows)
        int j0 = R.done, j1 = j0;
        while (j1 < n_sel && R.rows_sel[j1] < R.chunk0 + n_rows) j1++;
        if (j1 > j0) {
            for (int j = j0; j < j1; j++) m->pool_idx.pin[j] = R.rows_sel[j] - R.chunk0;
            IFA_HIP_CHECK(hipMemcpyAsync(m->pool_idx.dev + j0, m->pool_idx.pin + j0, sizeof(int) * (size_t)(j1 - j0), hipMemcpyHostToDevice, m->stream));
            if (!adj) {
                if ((rc = pool_rows_launch(m, logits, m->pool_idx.dev + j0, j0, j1, false))) return rc;
            } else {                   // runs of armed / raw rows, each run its own launches (all armed, the usual case: one run)
                for (int j = j0; j < j1; j++) slot_pin[j] = std::max(R.adj[(size_t)j], 0);
                IFA_HIP_CHECK(hipMemcpyAsync(slot_dev + j0, slot_pin + j0, sizeof(int) * (size_t)(j1 - j0), hipMemcpyHostToDevice, m->stream));
                for (int ja = j0; ja < j1;) {
                    const bool armed = R.adj[(size_t)ja] >= 0;
                    int jb = ja + 1;
                    while (jb < j1 && (R.adj[(size_t)jb] >= 0) == armed) jb++;
                    if ((rc = pool_rows_launch(m, logits, m->pool_idx.dev + ja, ja, jb, armed))) return rc;
                    ja = jb;
                }
            }
        }
        R.done = j1;
        if (!R.last_chunk) return IFA_OK;
    }
    IFA_HIP_CHECK(hipMemcpyAsync(m->pool_blk.pin, m->pool_blk.dev, pool_block_bytes(n_sel, k, R.lse), hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

// arms the request; an error code + message if this worker cannot serve it
static int pool_arm(ifa_model *m, int k, int n_sel, const int *rows_sel, const char *who)
{
    // what ifa_model_pool_adjust armed belongs to THIS step, whether it gets as far as a launch or not
    std::vector<int> adj;
    adj.swap(m->pool_adj_next);
    if (std::all_of(adj.begin(), adj.end(), [](int s) { return s < 0; })) adj.clear();
    IFA_REQUIRE(adj.empty() || (int)adj.size() == n_sel, "%s: ifa_model_pool_adjust armed %zu rows, the step pools %d", who, adj.size(), n_sel);
    IFA_REQUIRE(k >= 1 && k <= IFA_POOL_MAX, "%s: k %d outside 1..%d", who, k, IFA_POOL_MAX);
    if (m->cfg.tp_size > 1 || m->topo) return ifa_fail(IFA_ERR_STATE, "%s: the vocabulary of a partitioned worker is sharded; the pool is built on the host there", who);
    if (!m->g[T_LM_HEAD].present()) return ifa_fail(IFA_ERR_STATE, "%s: lm_head missing (pipeline stage worker)", who);
    IFA_HIP_CHECK(hipSetDevice(m->cfg.device));
    int rc = pool_reserve(m, n_sel, k);
    if (rc) return rc;
    if (m->opt_pool_lse && (rc = lse_part_reserve(m))) return rc;
    m->pool_lse_last.clear();
    m->pool = ifa_model::PoolReq();
    m->pool.lse = m->opt_pool_lse != 0;
    m->pool.k = k; m->pool.n_sel = n_sel; m->pool.rows_sel = rows_sel;
    if (!adj.empty()) {
        const size_t V = m->g[T_LM_HEAD].rows;
        for (int s : adj)
            if (s >= 0 && (size_t)s >= m->la_slots) { m->pool = ifa_model::PoolReq(); return ifa_fail(IFA_ERR_STATE, "%s: state slot %d has no logit state (ifa_model_logit_state_reset first)", who, s); }
        if ((size_t)n_sel * V > m->la_adj.cap()) {
            IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
            const size_t rows = (size_t)std::max(n_sel, 8);
            if (m->la_adj.alloc(rows * V)) { m->pool = ifa_model::PoolReq(); return ifa_fail(IFA_ERR_NOMEM, "%s: no memory for %zu adjusted rows", who, rows); }
        }
        m->pool.adj.swap(adj);
    }
    return IFA_OK;
}

// a pool entry point consumes what ifa_model_pool_adjust armed on EVERY way out, the argument checks in front of pool_arm included
struct AdjConsume { ifa_model *m; ~AdjConsume() { if (m) m->pool_adj_next.clear(); } };

// ---- device-fed batched steps (ifa_engine_batch_steps.hip): the rows and their state slots are the same for every step of the
// call, so they go to the device once; a step enqueues pool_enqueue's launches for a batched step and copies nothing to the host
int pool_fed_begin(ifa_model *m, int k, int n_sel, const int *rows_sel, const int *adj_slots, const char *who)
{
    AdjConsume consume{m};
    m->pool_adj_next.assign(adj_slots, adj_slots + n_sel);
    int rc = pool_arm(m, k, n_sel, rows_sel, who);
    if (rc) return rc;
    m->pool.lse = false;               // (no step of the call hands a log-sum-exp to anybody)
    int *slot_pin = m->pool_idx.pin + pool_idx_rows(m), *slot_dev = m->pool_idx.dev + pool_idx_rows(m);
    for (int j = 0; j < n_sel; j++) { m->pool_idx.pin[j] = rows_sel[j]; slot_pin[j] = std::max(adj_slots[j], 0); }
    hipError_t e = hipMemcpyAsync(m->pool_idx.dev, m->pool_idx.pin, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice, m->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(slot_dev, slot_pin, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice, m->stream);
    if (e != hipSuccess) { m->pool = ifa_model::PoolReq(); return ifa_fail(IFA_ERR_HIP, "%s: upload of the pooled rows failed: %s", who, hipGetErrorString(e)); }
    return IFA_OK;
}

int pool_fed_enqueue(ifa_model *m, const half_t *logits)
{
    const ifa_model::PoolReq &R = m->pool;
    if (R.adj.empty()) return pool_rows_launch(m, logits, m->pool_idx.dev, 0, R.n_sel, false);
    int rc;
    for (int ja = 0; ja < R.n_sel;) {      // runs of armed / raw rows, as in pool_enqueue
        const bool armed = R.adj[(size_t)ja] >= 0;
        int jb = ja + 1;
        while (jb < R.n_sel && (R.adj[(size_t)jb] >= 0) == armed) jb++;
        if ((rc = pool_rows_launch(m, logits, m->pool_idx.dev + ja, ja, jb, armed))) return rc;
        ja = jb;
    }
    return IFA_OK;
}

void pool_fed_block(ifa_model *m, int **counts, int **ids, void **vals)
{
    *counts = (int *)m->pool_blk.dev.get();
    *ids = *counts + m->pool.n_sel;
    *vals = *ids + (size_t)m->pool.n_sel * m->pool.k;
}

void pool_fed_end(ifa_model *m) { m->pool = ifa_model::PoolReq(); }

// after the step: disarms; copies the staged block out if the step succeeded and every wanted row was served
static int pool_finish(ifa_model *m, int step_rc, int *ids_host, unsigned short *vals_host, int *counts_host, const char *who)
{
    const ifa_model::PoolReq R = m->pool;
    m->pool = ifa_model::PoolReq();
    if (step_rc) return step_rc;
    if (R.done != R.n_sel) return ifa_fail(IFA_ERR_STATE, "%s: the step served %d of %d pools", who, R.done, R.n_sel);
    const int *counts = (const int *)m->pool_blk.pin.get(), *ids = counts + (R.lse ? 2 : 1) * R.n_sel;
    if (R.lse) m->pool_lse_last.assign((const float *)(counts + R.n_sel), (const float *)(counts + R.n_sel) + R.n_sel);
    const uint16_t *vals = (const uint16_t *)(ids + (size_t)R.n_sel * R.k);
    memcpy(counts_host, counts, sizeof(int) * (size_t)R.n_sel);
    memcpy(ids_host, ids, sizeof(int) * (size_t)R.n_sel * R.k);
    memcpy(vals_host, vals, sizeof(uint16_t) * (size_t)R.n_sel * R.k);
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
    int rc = logit_partitioned(m, who);
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
    int rc = logit_partitioned(m, who);
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
    int rc = logit_partitioned(m, who);
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
    AdjConsume consume{m};
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode_pool: model not finalized");
    IFA_REQUIRE(pool_ids_host && pool_vals_host && pool_count_host, "ifa_model_decode_pool: null pointer");
    int rc = pool_arm(m, k, 1, nullptr, "ifa_model_decode_pool");
    if (rc) return rc;
    int next = -1;
    rc = ifa_model_decode(m, token, pos, 1, &next, nullptr);
    rc = pool_finish(m, rc, pool_ids_host, pool_vals_host, pool_count_host, "ifa_model_decode_pool");
    if (!rc && next_token_host) *next_token_host = next;
    return rc;
}

int ifa_model_forward_pool(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev, int k,
                           int *next_token_host, int *pool_ids_host, unsigned short *pool_vals_host, int *pool_count_host)
{
    AdjConsume consume{m};
    IFA_REQUIRE(m && m->finalized, "ifa_model_forward_pool: model not finalized");
    IFA_REQUIRE(tokens_host && n_tokens >= 1 && pool_ids_host && pool_vals_host && pool_count_host, "ifa_model_forward_pool: bad arguments");
    int rc = pool_arm(m, k, 1, nullptr, "ifa_model_forward_pool");
    if (rc) return rc;
    int next = -1;
    rc = ifa_model_forward(m, tokens_host, n_tokens, prefix_len, logits_out_dev, &next);
    // (option exact_order feeds a prompt row by row: every row's step stages its pool, the last one's is what remains)
    rc = pool_finish(m, rc, pool_ids_host, pool_vals_host, pool_count_host, "ifa_model_forward_pool");
    if (!rc && next_token_host) *next_token_host = next;
    return rc;
}

int ifa_model_decode_batch_pool(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                                int *next_tokens_host, int k, const int *rows_sel_host, int n_sel,
                                int *pool_ids_host, unsigned short *pool_vals_host, int *pool_counts_host)
{
    AdjConsume consume{m};
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode_batch_pool: model not finalized");
    IFA_REQUIRE(n >= 1 && n_sel >= 0 && n_sel <= n, "ifa_model_decode_batch_pool: n %d n_sel %d", n, n_sel);
    if (n_sel == 0) { m->pool_adj_next.clear(); return ifa_model_decode_batch(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, nullptr); }
    IFA_REQUIRE(rows_sel_host && pool_ids_host && pool_vals_host && pool_counts_host, "ifa_model_decode_batch_pool: null pointer");
    for (int j = 0; j < n_sel; j++)
        IFA_REQUIRE(rows_sel_host[j] >= 0 && rows_sel_host[j] < n && (j == 0 || rows_sel_host[j] > rows_sel_host[j - 1]),
                    "ifa_model_decode_batch_pool: rows_sel must be strictly ascending indices below n = %d", n);
    if (m->opt_exact_order) return ifa_fail(IFA_ERR_STATE, "ifa_model_decode_batch_pool: option exact_order steps the rows one by one; take ifa_model_decode_pool per query");
    int rc = pool_arm(m, k, n_sel, rows_sel_host, "ifa_model_decode_batch_pool");
    if (rc) return rc;
    rc = ifa_model_decode_batch(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, nullptr);
    return pool_finish(m, rc, pool_ids_host, pool_vals_host, pool_counts_host, "ifa_model_decode_batch_pool");
}

} // extern "C"
