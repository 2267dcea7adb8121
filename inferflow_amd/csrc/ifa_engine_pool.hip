// ifa_engine_pool.hip -- worker steps that end in a candidate pool (ifa_model_decode_pool / _decode_batch_pool / _forward_pool):
// the entry point arms m->pool, runs the ordinary step -- whatever route ifa_model_decode / _decode_batch / _forward takes for
// this model -- and that step calls pool_enqueue() on its logits in front of its one stream synchronisation: one more launch
// (csrc/ifa_topk_pool.hip) and one copy of (counts, ids, values) into pinned staging.  Nothing is captured: the pool launch
// follows the graph replay on the stream.
#include "ifa_engine_state.h"

namespace ifa {
int topk_pool_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, int k, const unsigned *excl,
                   int *ids_out, void *vals_out, int *count_out, hipStream_t s);
int lse_rows(const void *logits, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n, const int *targets_dev, float *lse_out,
             float *target_out, float *part_dev, hipStream_t s);
}

namespace ifae {

// counts [n_sel] | (with_lse: lse [n_sel] |) ids [n_sel][k] | F16 bits [n_sel][k]
static size_t pool_block_bytes(int n_sel, int k, bool with_lse) { return (size_t)n_sel * (with_lse ? 8 : 4) + (size_t)n_sel * (size_t)k * 6; }

void pool_free(ifa_model *m)
{
    if (m->pool_excl) (void)hipFree(m->pool_excl);
    if (m->pool_dev) (void)hipFree(m->pool_dev);
    if (m->pool_pin) (void)hipHostFree(m->pool_pin);
    if (m->pool_idx_dev) (void)hipFree(m->pool_idx_dev);
    if (m->pool_idx_pin) (void)hipHostFree(m->pool_idx_pin);
    m->pool_excl = nullptr; m->pool_dev = m->pool_pin = nullptr; m->pool_idx_dev = m->pool_idx_pin = nullptr;
    m->pool_bytes = 0; m->pool_idx_cap = 0;
}

// staging for n_sel rows of k entries (grown on demand, outside any capture; one allocation serves every later step)
static int pool_reserve(ifa_model *m, int n_sel, int k)
{
    const size_t bytes = pool_block_bytes(std::max(n_sel, 8), IFA_POOL_MAX >= k ? IFA_POOL_MAX : k, true);
    if (bytes > m->pool_bytes) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if (m->pool_dev) (void)hipFree(m->pool_dev);
        if (m->pool_pin) (void)hipHostFree(m->pool_pin);
        m->pool_dev = m->pool_pin = nullptr; m->pool_bytes = 0;
        IFA_HIP_CHECK(hipMalloc(&m->pool_dev, bytes));
        IFA_HIP_CHECK(hipHostMalloc(&m->pool_pin, bytes, hipHostMallocDefault));
        m->pool_bytes = bytes;
    }
    if ((size_t)n_sel > m->pool_idx_cap) {
        IFA_HIP_CHECK(hipStreamSynchronize(m->stream));
        if (m->pool_idx_dev) (void)hipFree(m->pool_idx_dev);
        if (m->pool_idx_pin) (void)hipHostFree(m->pool_idx_pin);
        m->pool_idx_dev = m->pool_idx_pin = nullptr; m->pool_idx_cap = 0;
        const size_t cap = (size_t)std::max(n_sel, 64);
        IFA_HIP_CHECK(hipMalloc((void **)&m->pool_idx_dev, cap * sizeof(int)));
        IFA_HIP_CHECK(hipHostMalloc((void **)&m->pool_idx_pin, cap * sizeof(int), hipHostMallocDefault));
        m->pool_idx_cap = cap;
    }
    return IFA_OK;
}

int pool_enqueue(ifa_model *m, const half_t *logits, int n_rows)
{
    ifa_model::PoolReq &R = m->pool;
    if (R.k <= 0) return IFA_OK;
    const size_t V = m->g[T_LM_HEAD].rows;
    const int k = R.k, n_sel = R.n_sel;
    int *counts = (int *)m->pool_dev;
    float *lse = R.lse ? (float *)(counts + n_sel) : nullptr;
    int *ids = counts + (R.lse ? 2 : 1) * n_sel;
    uint16_t *vals = (uint16_t *)(ids + (size_t)n_sel * k);
    int rc = IFA_OK;
    if (!R.rows_sel) {                 // a single-query step: its one row
        if ((rc = topk_pool_rows(logits, V, nullptr, 1, V, k, m->pool_excl, ids, vals, counts, m->stream))) return rc;
        if (lse && (rc = lse_rows(logits, V, nullptr, 1, V, nullptr, lse, nullptr, m->lse_part, m->stream))) return rc;
        R.done = 1;
    } else {                           // a batched step (or one chunk of it): the wanted rows among [chunk0, chunk0 + n_rows)
        int j0 = R.done, j1 = j0;
        while (j1 < n_sel && R.rows_sel[j1] < R.chunk0 + n_rows) j1++;
        if (j1 > j0) {
            for (int j = j0; j < j1; j++) m->pool_idx_pin[j] = R.rows_sel[j] - R.chunk0;
            IFA_HIP_CHECK(hipMemcpyAsync(m->pool_idx_dev + j0, m->pool_idx_pin + j0, sizeof(int) * (size_t)(j1 - j0), hipMemcpyHostToDevice, m->stream));
            if ((rc = topk_pool_rows(logits, V, m->pool_idx_dev + j0, (size_t)(j1 - j0), V, k, m->pool_excl, ids + (size_t)j0 * k, vals + (size_t)j0 * k,
                                     counts + j0, m->stream))) return rc;
            if (lse && (rc = lse_rows(logits, V, m->pool_idx_dev + j0, (size_t)(j1 - j0), V, nullptr, lse + j0, nullptr, m->lse_part, m->stream))) return rc;
        }
        R.done = j1;
        if (!R.last_chunk) return IFA_OK;
    }
    IFA_HIP_CHECK(hipMemcpyAsync(m->pool_pin, m->pool_dev, pool_block_bytes(n_sel, k, R.lse), hipMemcpyDeviceToHost, m->stream));
    return IFA_OK;
}

// arms the request; an error code + message if this worker cannot serve it
static int pool_arm(ifa_model *m, int k, int n_sel, const int *rows_sel, const char *who)
{
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
    return IFA_OK;
}

// after the step: disarms; copies the staged block out if the step succeeded and every wanted row was served
static int pool_finish(ifa_model *m, int step_rc, int *ids_host, unsigned short *vals_host, int *counts_host, const char *who)
{
    const ifa_model::PoolReq R = m->pool;
    m->pool = ifa_model::PoolReq();
    if (step_rc) return step_rc;
    if (R.done != R.n_sel) return ifa_fail(IFA_ERR_STATE, "%s: the step served %d of %d pools", who, R.done, R.n_sel);
    const int *counts = (const int *)m->pool_pin, *ids = counts + (R.lse ? 2 : 1) * R.n_sel;
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
    if (n == 0) {
        if (m->pool_excl) (void)hipFree(m->pool_excl);
        m->pool_excl = nullptr;
        return IFA_OK;
    }
    std::vector<unsigned> bits(words, 0u);
    for (int i = 0; i < n; i++) bits[(size_t)ids_host[i] >> 5] |= 1u << (ids_host[i] & 31);
    if (!m->pool_excl) IFA_HIP_CHECK(hipMalloc((void **)&m->pool_excl, words * sizeof(unsigned)));
    IFA_HIP_CHECK(hipMemcpy(m->pool_excl, bits.data(), words * sizeof(unsigned), hipMemcpyHostToDevice));
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
    IFA_REQUIRE(m && m->finalized, "ifa_model_decode_batch_pool: model not finalized");
    IFA_REQUIRE(n >= 1 && n_sel >= 0 && n_sel <= n, "ifa_model_decode_batch_pool: n %d n_sel %d", n, n_sel);
    if (n_sel == 0) return ifa_model_decode_batch(m, n, tokens_host, positions_host, kv_slots_host, next_tokens_host, nullptr);
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
