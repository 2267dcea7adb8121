// engine_capi.cc -- C ABI of the InferenceEngine facade (include/inferflow_engine.h)
#include <algorithm>
#include <chrono>
#include <cstring>
#include <future>
#include <map>
#include <string>

#include "inferflow_engine.h"
#include "inference_engine.h"
#include "inferflow_service.h"
#include "perplexity.h"
#include "prefix_cache.h"
#include "step_plan.h"
#include "lookup_draft.h"
#include "context_shift.h"
#include "half_bits.h"

using namespace inferflow_amd;

struct ifa_engine {
    InferenceEngine engine;
    std::map<int, QueryInferenceResult> last;     // per query: result of the most recent step
    InferencePerfStat last_perf;                  // perf_stat of the most recent Infer()
};

extern "C" {

const char *ifa_engine_last_error(void) { return EngineLastError(); }

ifa_engine *ifa_engine_create(const char *ini_path, const char *section, const char *data_root_dir)
{
    if (!ini_path || !section) { EngineSetError("ifa_engine_create: null argument"); return nullptr; }
    InferenceConfig cfg;
    if (!InferenceEngine::LoadConfig(cfg, ini_path, section, data_root_dir ? data_root_dir : "")) return nullptr;
    ifa_engine *e = new ifa_engine();
    if (!e->engine.Init(cfg)) { delete e; return nullptr; }
    return e;
}

void ifa_engine_destroy(ifa_engine *e) { delete e; }

int ifa_engine_add_query(ifa_engine *e, const int *tokens, int n_tokens)
{
    if (!e || !tokens || n_tokens <= 0) { EngineSetError("ifa_engine_add_query: bad arguments"); return -1; }
    return e->engine.AddQuery(std::vector<int>(tokens, tokens + n_tokens), QueryOptions());
}

int ifa_engine_add_query_ex(ifa_engine *e, const int *tokens, int n_tokens, int strategy_id, int random_seed, float temperature)
{
    if (!e || !tokens || n_tokens <= 0) { EngineSetError("ifa_engine_add_query_ex: bad arguments"); return -1; }
    QueryOptions opt; opt.strategy_id = strategy_id; opt.random_seed = random_seed; opt.temperature = temperature;
    return e->engine.AddQuery(std::vector<int>(tokens, tokens + n_tokens), opt);
}

int ifa_engine_add_query_lp(ifa_engine *e, const int *tokens, int n_tokens, int strategy_id, int random_seed, float temperature, int logprobs)
{
    if (!e || !tokens || n_tokens <= 0) { EngineSetError("ifa_engine_add_query_lp: bad arguments"); return -1; }
    QueryOptions opt; opt.strategy_id = strategy_id; opt.random_seed = random_seed; opt.temperature = temperature; opt.logprobs = logprobs;
    return e->engine.AddQuery(std::vector<int>(tokens, tokens + n_tokens), opt);
}

int ifa_engine_add_query_opt(ifa_engine *e, const int *tokens, int n_tokens, const ifa_query_options *o)
{
    if (!e || !tokens || n_tokens <= 0 || !o) { EngineSetError("ifa_engine_add_query_opt: bad arguments"); return -1; }
    if (o->struct_size < sizeof(size_t)) { EngineSetError("ifa_engine_add_query_opt: struct_size %zu", o->struct_size); return -1; }
    ifa_query_options v;           // the caller's leading struct_size bytes over the defaults
    memset(&v, 0, sizeof v);
    v.temperature = 1.0f; v.logprobs = -1; v.repetition_penalty = 1.0f; v.context_shift = -1; v.context_keep = -1;
    memcpy(&v, o, std::min(o->struct_size, sizeof v));
    if (v.n_logit_bias < 0 || (v.n_logit_bias > 0 && (!v.logit_bias_ids || !v.logit_bias_values))) { EngineSetError("ifa_engine_add_query_opt: %d logit_bias entries without arrays", v.n_logit_bias); return -1; }
    QueryOptions opt; opt.strategy_id = v.strategy_id; opt.random_seed = v.random_seed; opt.temperature = v.temperature; opt.logprobs = v.logprobs;
    opt.repetition_penalty = v.repetition_penalty; opt.presence_penalty = v.presence_penalty; opt.frequency_penalty = v.frequency_penalty;
    for (int i = 0; i < v.n_logit_bias; i++) opt.logit_bias.emplace_back(v.logit_bias_ids[i], v.logit_bias_values[i]);
    opt.context_shift = v.context_shift; opt.context_keep = v.context_keep;
    return e->engine.AddQuery(std::vector<int>(tokens, tokens + n_tokens), opt);
}

int ifa_engine_last_logprobs(ifa_engine *e, int query_id, float *chosen, int *ids, float *logprobs, int cap, int *n)
{
    if (!e || cap < 0 || (cap > 0 && (!ids || !logprobs))) { EngineSetError("ifa_engine_last_logprobs: bad arguments"); return 0; }
    auto it = e->last.find(query_id);
    if (it == e->last.end()) { EngineSetError("no result for query %d", query_id); return 0; }
    if (!it->second.has_logprobs) { EngineSetError("query %d was added without logprobs", query_id); return 0; }
    if (chosen) *chosen = it->second.chosen_logprob;
    const int m = (int)it->second.top_logprobs.size();
    for (int i = 0; i < std::min(m, cap); i++) { ids[i] = it->second.top_logprobs[(size_t)i].id; logprobs[i] = it->second.top_logprobs[(size_t)i].weight; }
    if (n) *n = m;
    return 1;
}

int ifa_engine_score(ifa_engine *e, const int *tokens, int n_tokens, float *logprobs_out)
{
    if (!e || !tokens || n_tokens < 2 || !logprobs_out) { EngineSetError("ifa_engine_score: bad arguments"); return 0; }
    std::vector<float> lp;
    if (!e->engine.ScoreTokens(std::vector<int>(tokens, tokens + n_tokens), lp)) return 0;
    memcpy(logprobs_out, lp.data(), sizeof(float) * lp.size());
    return 1;
}

int ifa_engine_strategy_id(ifa_engine *e, const char *name)
{
    return (int)(e ? e->engine.GetSamplingStrategyId(name ? name : "") : SamplingStrategyIdFromName(name ? name : ""));
}

int ifa_sampling_choose(const uint16_t *logits_f16, int vocab, int strategy_id, int max_k, float top_p, int pool_size,
                        float temperature, long long seed, int n_draws, int *out_ids, float *out_probs,
                        int *pool_ids, float *pool_probs, int pool_capacity)
{
    if (!logits_f16 || vocab <= 0 || n_draws < 0) { EngineSetError("ifa_sampling_choose: bad arguments"); return -1; }
    StdSamplingConfig cfg; cfg.max_k = max_k; cfg.top_p = top_p; cfg.pool_size = pool_size;
    JavaRandom rng((uint64_t)seed);
    int pool_n = 0;
    for (int d = 0; d < std::max(1, n_draws); d++) {
        SamplingOutput out; SamplingState st;
        if (!IsStdFamily((SamplingStrategyId)strategy_id) || !ChooseTokens(out, logits_f16, vocab, (SamplingStrategyId)strategy_id, cfg, temperature, rng, st)) { EngineSetError("ifa_sampling_choose: unsupported strategy %d", strategy_id); return -1; }
        if (d < n_draws && !out.selected.empty()) { if (out_ids) out_ids[d] = out.selected[0].id; if (out_probs) out_probs[d] = out.selected[0].weight; }
        pool_n = (int)out.token_pool.size();
        for (int i = 0; i < pool_n && i < pool_capacity; i++) { if (pool_ids) pool_ids[i] = out.token_pool[(size_t)i].id; if (pool_probs) pool_probs[i] = out.token_pool[(size_t)i].weight; }
    }
    return pool_n;
}

double ifa_perplexity_token_nll(const uint16_t *logits_f16, int vocab, int token_id)
{
    if (!logits_f16 || vocab <= 0 || token_id < 0 || token_id >= vocab) { EngineSetError("ifa_perplexity_token_nll: bad arguments"); return -1.0; }
    return TokenNll(logits_f16, vocab, token_id);
}

int ifa_sampling_choose_ex(const uint16_t *logits_f16, int vocab, int strategy_id, const float *params9, float temperature,
                           long long seed, int n_draws, int *out_ids, float *out_probs, int *pool_ids, float *pool_probs,
                           int pool_capacity, float *mirostat_mu_inout, const int *text_tokens, int n_text)
{
    if (!logits_f16 || vocab <= 0 || n_draws < 0 || !params9) { EngineSetError("ifa_sampling_choose_ex: bad arguments"); return -1; }
    SamplingConfig cfg;
    cfg.max_k = (int)params9[0]; cfg.top_p = params9[1]; cfg.pool_size = (int)params9[2]; cfg.min_p = params9[3]; cfg.tfs_z = params9[4];
    cfg.typical_p = params9[5]; cfg.mirostat_eta = params9[6]; cfg.mirostat_tau = params9[7]; cfg.eos_bypassing_max = (int)params9[8];
    cfg.rfsd_top_p = cfg.top_p;            // (RandomizedFSD's sampling branch has its own top_p: 0.93 by default, here the caller's)
    JavaRandom rng((uint64_t)seed);
    SamplingState st;
    if (mirostat_mu_inout) st.mirostat_mu = *mirostat_mu_inout;
    const std::vector<int> text(text_tokens, text_tokens + (text_tokens ? std::max(0, n_text) : 0));
    int pool_n = 0;
    for (int d = 0; d < std::max(1, n_draws); d++) {
        SamplingOutput out;
        if (!ChooseTokens(out, logits_f16, vocab, (SamplingStrategyId)strategy_id, cfg, temperature, rng, st, text)) { EngineSetError("ifa_sampling_choose_ex: unsupported strategy %d", strategy_id); return -1; }
        if (d < n_draws && !out.selected.empty()) { if (out_ids) out_ids[d] = out.selected[0].id; if (out_probs) out_probs[d] = out.selected[0].weight; }
        pool_n = (int)out.token_pool.size();
        for (int i = 0; i < pool_n && i < pool_capacity; i++) { if (pool_ids) pool_ids[i] = out.token_pool[(size_t)i].id; if (pool_probs) pool_probs[i] = out.token_pool[(size_t)i].weight; }
    }
    if (mirostat_mu_inout) *mirostat_mu_inout = st.mirostat_mu;
    return pool_n;
}

int ifa_sampling_choose_from_pool(const int *cand_ids, const uint16_t *cand_vals_f16, int cand_count, int strategy_id, const float *params9,
                                  float temperature, long long seed, int n_draws, int *out_ids, float *out_probs, int *pool_ids,
                                  float *pool_probs, int pool_capacity, float *mirostat_mu_inout, const int *text_tokens, int n_text)
{
    if (cand_count < 0 || (cand_count > 0 && (!cand_ids || !cand_vals_f16)) || n_draws < 0 || !params9) { EngineSetError("ifa_sampling_choose_from_pool: bad arguments"); return -1; }
    SamplingConfig cfg;
    cfg.max_k = (int)params9[0]; cfg.top_p = params9[1]; cfg.pool_size = (int)params9[2]; cfg.min_p = params9[3]; cfg.tfs_z = params9[4];
    cfg.typical_p = params9[5]; cfg.mirostat_eta = params9[6]; cfg.mirostat_tau = params9[7]; cfg.eos_bypassing_max = (int)params9[8];
    cfg.rfsd_top_p = cfg.top_p;
    std::vector<IdWeight> cand((size_t)cand_count);
    for (int i = 0; i < cand_count; i++) { cand[(size_t)i].id = cand_ids[i]; cand[(size_t)i].weight = HalfBitsToFloat(cand_vals_f16[i]); }
    JavaRandom rng((uint64_t)seed);
    SamplingState st;
    if (mirostat_mu_inout) st.mirostat_mu = *mirostat_mu_inout;
    const std::vector<int> text(text_tokens, text_tokens + (text_tokens ? std::max(0, n_text) : 0));
    int pool_n = 0;
    for (int d = 0; d < std::max(1, n_draws); d++) {
        SamplingOutput out;
        if (!ChooseTokensFromPool(out, cand, (SamplingStrategyId)strategy_id, cfg, temperature, rng, st, text)) { EngineSetError("ifa_sampling_choose_from_pool: unsupported strategy %d", strategy_id); return -1; }
        if (d < n_draws && !out.selected.empty()) { if (out_ids) out_ids[d] = out.selected[0].id; if (out_probs) out_probs[d] = out.selected[0].weight; }
        pool_n = (int)out.token_pool.size();
        for (int i = 0; i < pool_n && i < pool_capacity; i++) { if (pool_ids) pool_ids[i] = out.token_pool[(size_t)i].id; if (pool_probs) pool_probs[i] = out.token_pool[(size_t)i].weight; }
    }
    if (mirostat_mu_inout) *mirostat_mu_inout = st.mirostat_mu;
    return pool_n;
}

int ifa_sampling_random_doubles(long long seed, int n, double *out)
{
    if (!out || n < 0) return 0;
    JavaRandom rng((uint64_t)seed);
    for (int i = 0; i < n; i++) out[i] = rng.NextDouble();
    return n;
}

int ifa_engine_query_count(ifa_engine *e) { return e ? e->engine.QueryCount() : -1; }

int ifa_engine_remove_query(ifa_engine *e, int query_id)
{
    if (!e) return 0;
    e->last.erase(query_id);
    return e->engine.RemoveQuery(query_id) ? 1 : 0;
}

int ifa_engine_infer(ifa_engine *e, int *query_ids, int *next_tokens, int capacity)
{
    if (!e) { EngineSetError("ifa_engine_infer: null engine"); return -1; }
    InferenceResult res;
    if (!e->engine.Infer(res)) return -1;
    e->last_perf = res.perf_stat;
    int n = 0;
    for (QueryInferenceResult &item : res.items) {
        if (n < capacity && query_ids && next_tokens) { query_ids[n] = item.query_id; next_tokens[n] = item.next_tokens.empty() ? -1 : item.next_tokens[0].id; }
        n++;
        e->last[item.query_id] = std::move(item);
    }
    return n;
}

int ifa_engine_perf_stat(ifa_engine *e, unsigned *keys, float *ms, int capacity)
{
    if (!e) { EngineSetError("ifa_engine_perf_stat: null engine"); return -1; }
    int n = 0;
    for (const auto &kv : e->last_perf.time_map) {
        if (n < capacity && keys && ms) { keys[n] = kv.first; ms[n] = kv.second; }
        n++;
    }
    return n;
}

int ifa_engine_commit(ifa_engine *e, const int *query_ids, const int *tokens, const int *is_end, int n)
{
    if (!e || !query_ids || !tokens || n < 0) { EngineSetError("ifa_engine_commit: bad arguments"); return 0; }
    std::map<int, QueryNextToken> m;
    for (int i = 0; i < n; i++) { QueryNextToken t; t.id = tokens[i]; t.is_end = is_end && is_end[i]; m[query_ids[i]] = t; }
    return e->engine.CommitInferenceResult(m) ? 1 : 0;
}

int ifa_engine_last_logits(ifa_engine *e, int query_id, uint16_t *dst_f16, size_t capacity, int *rows, int *cols)
{
    if (!e) return 0;
    auto it = e->last.find(query_id);
    if (it == e->last.end()) { EngineSetError("no result for query %d", query_id); return 0; }
    if (rows) *rows = it->second.output_rows;
    if (cols) *cols = it->second.output_cols;
    if (dst_f16) memcpy(dst_f16, it->second.output_tensor.data(), std::min(capacity, it->second.output_tensor.size()) * 2);
    return 1;
}

int ifa_engine_generate(ifa_engine *e, int query_id, int n_steps, int *out_tokens, float *gpu_ms)
{
    if (!e || !out_tokens) { EngineSetError("ifa_engine_generate: bad arguments"); return -1; }
    std::vector<int> toks;
    if (!e->engine.Generate(query_id, n_steps, toks, gpu_ms)) return -1;
    for (size_t i = 0; i < toks.size(); i++) out_tokens[i] = toks[i];
    return (int)toks.size();
}

int ifa_engine_generate_lookup(ifa_engine *e, int query_id, int max_new, const int *prediction, int n_prediction, int *out_tokens, float *stats5)
{
    if (!e || !out_tokens || n_prediction < 0 || (n_prediction > 0 && !prediction)) { EngineSetError("ifa_engine_generate_lookup: bad arguments"); return -1; }
    std::vector<int> toks, pred;
    if (n_prediction > 0) pred.assign(prediction, prediction + n_prediction);
    LookupStats st;
    const bool ok = e->engine.GenerateLookup(query_id, max_new, toks, n_prediction > 0 ? &pred : nullptr, &st);
    if (stats5) { stats5[0] = (float)st.steps; stats5[1] = (float)st.draft_steps; stats5[2] = (float)st.drafted; stats5[3] = (float)st.accepted; stats5[4] = st.gpu_ms; }
    if (!ok) return -1;
    for (size_t i = 0; i < toks.size(); i++) out_tokens[i] = toks[i];
    return (int)toks.size();
}

int ifa_engine_generate_batch(ifa_engine *e, int n, const int *query_ids, const int *max_new, const int *stop_ids, const int *stop_offsets,
                              int *out_tokens, const int *out_offsets, int *counts, int *stopped, float *stats4)
{
    if (!e || n < 0 || (n > 0 && (!query_ids || !max_new || !out_tokens || !out_offsets || !counts || !stopped))) { EngineSetError("ifa_engine_generate_batch: bad arguments"); return -1; }
    std::vector<BatchGenerateItem> items((size_t)n);
    for (int i = 0; i < n; i++) {
        items[(size_t)i].query_id = query_ids[i]; items[(size_t)i].max_new_tokens = max_new[i];
        if (max_new[i] > out_offsets[i + 1] - out_offsets[i]) { EngineSetError("ifa_engine_generate_batch: query %d: room for %d of %d tokens", query_ids[i], out_offsets[i + 1] - out_offsets[i], max_new[i]); return -1; }
        if (stop_offsets) {
            if (stop_offsets[i + 1] < stop_offsets[i] || (stop_offsets[i + 1] > stop_offsets[i] && !stop_ids)) { EngineSetError("ifa_engine_generate_batch: stop offsets of query %d", query_ids[i]); return -1; }
            items[(size_t)i].stop_token_ids.assign(stop_ids + stop_offsets[i], stop_ids + stop_offsets[i + 1]);
        }
    }
    BatchGenerateStats st;
    const bool ok = e->engine.GenerateBatch(items, nullptr, &st);
    if (stats4) { stats4[0] = (float)st.rounds; stats4[1] = (float)st.batched_steps; stats4[2] = (float)st.single_steps; stats4[3] = st.gpu_ms; }
    if (!ok) return -1;
    for (int i = 0; i < n; i++) {
        const BatchGenerateItem &it = items[(size_t)i];
        counts[i] = (int)it.new_tokens.size(); stopped[i] = it.stopped ? 1 : 0;
        for (size_t t = 0; t < it.new_tokens.size(); t++) out_tokens[out_offsets[i] + (int)t] = it.new_tokens[t];
    }
    return 0;
}

// host-only: the rounds of GenerateBatch (host/step_plan.h)
int ifa_generate_batch_plan(const int *facts, int n_facts, int *out, int n_out)
{
    if (!facts || !out || n_facts < 7 || facts[6] < 0 || n_facts != 7 + 6 * facts[6] || n_out < 4 + 2 * facts[6]) { EngineSetError("ifa_generate_batch_plan: bad arguments"); return -1; }
    GenBatchFacts f;
    f.min_queries = facts[0]; f.round_steps = facts[1]; f.fused_max = facts[2]; f.device_sampler = facts[3] != 0; f.multi_gpu = facts[4] != 0; f.return_output_tensors = facts[5] != 0;
    std::vector<GenBatchQuery> qs((size_t)facts[6]);
    for (size_t i = 0; i < qs.size(); i++) {
        const int *q = facts + 7 + 6 * i;
        if (q[4] < 0 || q[4] > 2) { EngineSetError("ifa_generate_batch_plan: query %d: kind %d", q[0], q[4]); return -1; }
        qs[i].id = q[0]; qs[i].remaining = q[1]; qs[i].room = q[2]; qs[i].shift_on = q[3] != 0; qs[i].kind = (GenKind)q[4]; qs[i].has_stops = q[5] != 0;
    }
    const GenBatchPlan p = PlanGenerateBatch(f, qs);
    out[0] = (int)p.refusal; out[1] = p.refused_id; out[2] = (int)p.route; out[3] = (int)p.ids.size();
    for (size_t i = 0; i < p.ids.size(); i++) { out[4 + 2 * i] = p.ids[i]; out[5 + 2 * i] = p.steps[i]; }
    return 0;
}

// host-only: the draft of lookup decoding (host/lookup_draft.h)
int ifa_lookup_draft(const int *ctx, int n_ctx, const int *pred, int n_pred, int ngram_max, int ngram_min, int k, int *draft_out)
{
    const int n = LookupDraft(ctx, n_ctx, pred, n_pred, ngram_max, ngram_min, k, draft_out);
    if (n < 0) EngineSetError("ifa_lookup_draft: bad arguments");
    return n;
}

static int engine_perplexity(ifa_engine *e, const int *tokens, int n_tokens, int max_length, int stride, bool device_scoring,
                             double *ppl, double *ppl_stderr, long long *count)
{
    if (!e || !tokens || n_tokens <= 0) { EngineSetError("ifa_engine_perplexity: bad arguments"); return 0; }
    PerplexityResult r;
    if (!ComputePerplexity(e->engine, std::vector<int>(tokens, tokens + n_tokens), max_length, stride, r, 8, device_scoring)) return 0;
    if (ppl) *ppl = r.ppl;
    if (ppl_stderr) *ppl_stderr = r.ppl_stderr;
    if (count) *count = r.count;
    return 1;
}

int ifa_engine_perplexity(ifa_engine *e, const int *tokens, int n_tokens, int max_length, int stride,
                          double *ppl, double *ppl_stderr, long long *count)
{
    return engine_perplexity(e, tokens, n_tokens, max_length, stride, false, ppl, ppl_stderr, count);
}

int ifa_engine_perplexity_device(ifa_engine *e, const int *tokens, int n_tokens, int max_length, int stride,
                                 double *ppl, double *ppl_stderr, long long *count)
{
    return engine_perplexity(e, tokens, n_tokens, max_length, stride, true, ppl, ppl_stderr, count);
}

int ifa_engine_model_info(ifa_engine *e, const char *key)
{
    if (!e || !key) return -1;
    const ModelSpec &s = e->engine.model_spec();
    const std::string k = key;
    if (k == "vocab_size") return s.hyper_params.vocab_size;
    if (k == "embd_dims") return s.hyper_params.embd_dims;
    if (k == "hidden_dim") return s.hyper_params.hidden_dim;
    if (k == "decoder_layers") return s.hyper_params.decoder_layers;
    if (k == "decoder_heads") return s.hyper_params.decoder_heads;
    if (k == "decoder_kv_heads") return s.hyper_params.decoder_kv_heads;
    if (k == "max_context_len") return e->engine.MaxContextLen();
    if (k == "device_weight_data_type") return s.device_weight_data_type;
    if (k == "device_kv_cache_data_type") return s.device_kv_cache_data_type;
    if (k == "partition_ranks") return e->engine.PartitionRanks();
    if (k == "device_sampling_pool") return e->engine.config().device_sampling_pool ? 1 : 0;
    if (k == "sampled_fused_steps") return (int)std::min<long long>(e->engine.sampled_fused_steps(), 0x7FFFFFFF);
    if (k == "device_sampler") return e->engine.device_sampler_active() ? 1 : 0;
    if (k == "device_sampled_steps") return (int)std::min<long long>(e->engine.device_sampled_steps(), 0x7FFFFFFF);
    if (k == "prefix_cache") return e->engine.prefix_cache_active() ? 1 : 0;
    if (k == "prefix_cache_hits") return (int)std::min<long long>(e->engine.prefix_cache_hits(), 0x7FFFFFFF);
    if (k == "prefix_cache_tokens") return (int)std::min<long long>(e->engine.prefix_cache_tokens(), 0x7FFFFFFF);
    if (k == "lookup_decoding") return e->engine.lookup_decoding_active() ? 1 : 0;
    if (k == "lookup_sampled") return e->engine.lookup_sampled_active() ? 1 : 0;
    if (k == "lookup_sampled_steps") return (int)std::min<long long>(e->engine.lookup_sampled_steps(), 0x7FFFFFFF);
    if (k == "logit_processors") return e->engine.SupportsLogitProcessors() ? 1 : 0;
    if (k == "processed_steps") return (int)std::min<long long>(e->engine.processed_steps(), 0x7FFFFFFF);
    if (k == "context_shift") return e->engine.ShiftsContext() ? 1 : 0;
    if (k == "context_shift_available") return e->engine.SupportsContextShift() ? 1 : 0;
    if (k == "context_shifts") return (int)std::min<long long>(e->engine.context_shifts(), 0x7FFFFFFF);
    if (k == "context_shift_tokens") return (int)std::min<long long>(e->engine.context_shift_tokens(), 0x7FFFFFFF);
    if (k == "batch_generate") return e->engine.batch_generate_active() ? 1 : 0;
    if (k == "batch_generate_steps") return (int)std::min<long long>(e->engine.batch_generate_steps(), 0x7FFFFFFF);
    if (k == "batch_generate_rounds") return (int)std::min<long long>(e->engine.batch_generate_rounds(), 0x7FFFFFFF);
    if (k == "prefix_cache_copies") return (int)std::min<long long>(e->engine.prefix_cache_copies(), 0x7FFFFFFF);
    return -1;
}

int ifa_engine_query_cached_tokens(ifa_engine *e, int query_id) { return e ? e->engine.QueryCachedTokens(query_id) : -1; }

int ifa_engine_query_shifted_tokens(ifa_engine *e, int query_id) { return e ? e->engine.QueryShiftedTokens(query_id) : -1; }

int ifa_engine_query_rng_state(ifa_engine *e, int query_id, unsigned long long *state)
{
    if (!e || !state) { EngineSetError("ifa_engine_query_rng_state: bad arguments"); return 0; }
    return e->engine.QueryRngState(query_id, state) ? 1 : 0;
}

int ifa_engine_shift_query(ifa_engine *e, int query_id, int keep, int discard)
{
    if (!e) { EngineSetError("ifa_engine_shift_query: null engine"); return 0; }
    return e->engine.ShiftQuery(query_id, keep, discard) ? 1 : 0;
}

// host-only: the context shift's policy (host/context_shift.h)
int ifa_context_shift_plan(int n_tokens, int processed, int max_ctx, int keep, int *out2)
{
    ContextShiftPlan plan;
    if (!out2 || !PlanContextShift(n_tokens, processed, max_ctx, keep, plan)) { EngineSetError("ifa_context_shift_plan: bad arguments"); return -1; }
    if (!plan.shift) return 0;
    out2[0] = plan.keep; out2[1] = plan.discard;
    return 1;
}

// host-only: the slot / reuse plan of the prompt prefix cache (host/prefix_cache.h)
int ifa_prefix_cache_plan(const int *records_flat, const int *record_lens, const int *busy, const long long *stamps, int n_slots,
                          const int *prompt, int n_prompt, int min_tokens, int *out3)
{
    if (!record_lens || !busy || !stamps || n_slots < 1 || !prompt || n_prompt < 1 || min_tokens < 1 || !out3) { EngineSetError("ifa_prefix_cache_plan: bad arguments"); return -1; }
    std::vector<PrefixSlotView> views((size_t)n_slots);
    size_t off = 0;
    for (int i = 0; i < n_slots; i++) {
        if (record_lens[i] < 0 || (record_lens[i] > 0 && !records_flat)) { EngineSetError("ifa_prefix_cache_plan: record %d", i); return -1; }
        views[(size_t)i].record = records_flat ? records_flat + off : nullptr; views[(size_t)i].record_len = record_lens[i];
        views[(size_t)i].busy = busy[i] != 0; views[(size_t)i].stamp = stamps[i];
        off += (size_t)record_lens[i];
    }
    PrefixPlan plan;
    if (!PlanPrefixReuse(views, prompt, n_prompt, min_tokens, plan)) { EngineSetError("ifa_prefix_cache_plan: no free slot"); return -1; }
    out3[0] = plan.slot; out3[1] = plan.src_slot; out3[2] = plan.reuse_len;
    return 0;
}

// host-only: the route of an engine step (host/step_plan.h)
int ifa_step_plan_query(int multi, int return_output_tensors, int pool_route, int sampled, int n_new, int *out3)
{
    if (n_new < 1 || !out3) { EngineSetError("ifa_step_plan_query: bad arguments"); return -1; }
    const QueryStepPlan plan = PlanQueryStep(multi != 0, return_output_tensors != 0, pool_route != 0, sampled != 0, n_new);
    out3[0] = (int)plan.route; out3[1] = plan.logits_rows; out3[2] = (int)plan.copy;
    return 0;
}

int ifa_step_plan_batch(int return_output_tensors, const int *rows5, int n_rows, int *pool_rows_out, int *out5)
{
    if (!rows5 || n_rows < 1 || !pool_rows_out || !out5) { EngineSetError("ifa_step_plan_batch: bad arguments"); return -1; }
    std::vector<BatchRow> rows((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        const int *f = rows5 + (size_t)r * 5;
        if (f[2] < 0 || f[3] < 0) { EngineSetError("ifa_step_plan_batch: row %d", r); return -1; }
        rows[(size_t)r].pool_route = f[0] != 0; rows[(size_t)r].sampled = f[1] != 0; rows[(size_t)r].pool_len = f[2]; rows[(size_t)r].pool_k = f[3];
        rows[(size_t)r].wants_logprobs = f[4] != 0;
    }
    const BatchStepPlan plan = PlanBatchStep(return_output_tensors != 0, rows);
    for (size_t i = 0; i < plan.pool_rows.size(); i++) pool_rows_out[i] = plan.pool_rows[i];
    out5[0] = (int)plan.pool_rows.size(); out5[1] = plan.pool_k; out5[2] = plan.with_lse ? 1 : 0; out5[3] = plan.want_logits ? 1 : 0; out5[4] = plan.error_row;
    return 0;
}

// the worker (ifa_model *, for the ifa_model_* calls of include/inferflow_amd.h) of partition rank `rank` and its plan
// {stage, n_stages, tp_rank, tp_size, layer0, layer1}; null / -1 for a rank that does not exist
void *ifa_engine_worker(ifa_engine *e, int rank) { return e ? (void *)e->engine.worker(rank) : nullptr; }
int ifa_engine_worker_plan(ifa_engine *e, int rank, int *out6) { return e && out6 && e->engine.WorkerPlanOf(rank, out6) ? 0 : -1; }

// host-only: the partition rules of the multi-GPU engine (model_loader.cc) for tests and tools
int ifa_partition_slice(int stage, int n_stages, int tp_rank, int tp_size, int layer0, int layer1, int layer, int tensor_id,
                        size_t rows, size_t cols, size_t *out5)
{
    if (!out5) return -1;
    WorkerPlan w; w.stage = stage; w.n_stages = n_stages; w.tp_rank = tp_rank; w.tp_size = tp_size; w.layer0 = layer0; w.layer1 = layer1;
    w.first_stage = stage == 0; w.last_stage = stage + 1 == n_stages;
    TensorSlice sl;
    if (!SliceForWorker(w, layer, tensor_id, rows, cols, sl)) return 0;
    out5[0] = sl.row0; out5[1] = sl.row1; out5[2] = sl.col0; out5[3] = sl.col1; out5[4] = (size_t)sl.local_layer;
    return 1;
}

int ifa_partition_split_layers(int n_layers, int n_groups, int *out_pairs, int capacity_pairs)
{
    if (!out_pairs || n_groups < 1) return -1;
    std::vector<std::pair<int, int>> r;
    SplitGpuLayers(n_layers, n_groups, r);
    for (size_t i = 0; i < r.size() && (int)i < capacity_pairs; i++) { out_pairs[2 * i] = r[i].first; out_pairs[2 * i + 1] = r[i].second; }
    return (int)r.size();
}

// Service shell (host/inferflow_service.*), testable without a device: parses a request body the way the HTTP front does and
// writes the parsed fields back as one JSON object; returns 0, or -1 when the body is rejected / the buffer is too small
int ifa_service_parse_request(const char *body, int is_openai_mode, char *out_json, size_t cap)
{
    if (!body || !out_json || cap == 0) return -1;
    InferFlowRequest r;
    std::string err;
    if (!InferFlowServiceCore::ParseRequest(r, body, is_openai_mode != 0, &err)) { snprintf(out_json, cap, "{\"ret_code\": \"%s\"}", err.c_str()); return -1; }
    std::string ids = "[";
    for (size_t i = 0; i < r.prompt_token_ids.size(); i++) { if (i) ids += ", "; ids += std::to_string(r.prompt_token_ids[i]); }
    ids += "]";
    char tmp[64]; snprintf(tmp, sizeof tmp, "%.4f", r.temperature);
    const std::string js = "{\"prompt_token_ids\": " + ids + ", \"max_output_len\": " + std::to_string(r.max_output_len) + ", \"decoding_alg\": \"" + r.decoding_alg
        + "\", \"random_seed\": " + std::to_string(r.random_seed) + ", \"temperature\": " + tmp + ", \"is_streaming_mode\": " + (r.is_streaming_mode ? "true" : "false")
        + ", \"eos_token_id\": " + std::to_string(r.eos_token_id) + ", \"fn\": \"" + r.fn + "\""
        + (r.logprobs >= 0 ? ", \"logprobs\": " + std::to_string(r.logprobs) : std::string()) + r.ProcessorsJson() + "}";
    if (js.size() + 1 > cap) return -1;
    memcpy(out_json, js.c_str(), js.size() + 1);
    return 0;
}

// formats a response chunk (native or OpenAI shape) from token ids: the exact strings the HTTP front sends
int ifa_service_format_response(const int *token_ids, int n, int is_end, int is_openai_mode, int is_chunk, int prompt_tokens, char *out_json, size_t cap)
{
    if (!out_json || cap == 0 || n < 0 || (n > 0 && !token_ids)) return -1;
    InferFlowResponseChunk c;
    c.ret_code = "succ"; c.token_ids.assign(token_ids, token_ids + n); c.is_end = is_end != 0; c.prompt_tokens = prompt_tokens;
    std::string js;
    if (is_openai_mode) c.ToJsonOpenAI(js, is_chunk != 0, "ifa-test"); else c.ToJson(js);
    if (js.size() + 1 > cap) return -1;
    memcpy(out_json, js.c_str(), js.size() + 1);
    return 0;
}

// ---- the service LOOP without a device -------------------------------------------------------------------------------------------
// A host-only QueryEngine with InferenceEngine's query-table semantics (AddQuery: > 0 id / 0 busy / -1 too long; Infer: one item
// per query with uncommitted tokens, a query whose context is full is marked ended and gets NO item, a failed step returns false
// without items; Commit appends, is_end ends) over a trivial "model": next token = (last + 1) % vocab.
namespace {
struct LoopbackEngine : QueryEngine {
    struct Q { std::vector<int> tokens; int processed = 0; bool ended = false; int logprobs = -1; };
    std::map<int, Q> qs;
    int max_ctx, max_queries, fail_at, vocab = 1000, next_id = 1, infer_calls = 0;
    LoopbackEngine(int ctx, int mq, int fail) : max_ctx(ctx), max_queries(mq), fail_at(fail) {}
    int AddQuery(const std::vector<int> &t, const QueryOptions &o) override {
        if (t.empty() || (int)t.size() >= max_ctx) return -1;
        if (o.logprobs < -1 || o.logprobs > QueryOptions::MAX_LOGPROBS) return -1;       // (InferenceEngine::AddQuery's rule)
        if ((int)qs.size() >= max_queries) return 0;
        Q q; q.tokens = t; q.logprobs = o.logprobs; qs[next_id] = q; return next_id++;
    }
    bool SupportsLogprobs() const override { return true; }
    int QueryCount() const override { return (int)qs.size(); }
    bool Infer(InferenceResult &res) override {
        res.items.clear();
        ++infer_calls;
        if (infer_calls == fail_at) return false;                                        // fail_at = N > 0: call N fails once (a retry succeeds)
        if (fail_at < 0 && (infer_calls == -fail_at || infer_calls == -fail_at + 1)) return false;      // fail_at = -N: calls N and N + 1 fail (the retry too)
        for (auto &kv : qs) {
            Q &q = kv.second;
            if (q.ended) continue;
            if ((int)q.tokens.size() >= max_ctx) { q.ended = true; continue; }
            if ((int)q.tokens.size() - q.processed <= 0) continue;
            QueryInferenceResult item; item.query_id = kv.first; item.prefix_len = q.processed;
            IdWeight w; w.id = (q.tokens.back() + 1) % vocab; w.weight = 1.0f;
            item.next_tokens.push_back(w);
            if (q.logprobs >= 0) {           // a fixed "distribution": candidate j is (next + j) % vocab with log p = -0.25 - j
                item.has_logprobs = true; item.chosen_logprob = -0.25f;
                for (int j = 0; j < q.logprobs; j++) { IdWeight c; c.id = (w.id + j) % vocab; c.weight = -0.25f - (float)j; item.top_logprobs.push_back(c); }
            }
            q.processed = (int)q.tokens.size();
            res.items.push_back(item);
        }
        return true;
    }
    bool CommitInferenceResult(const std::map<int, QueryNextToken> &m) override {
        for (const auto &kv : m) { auto it = qs.find(kv.first); if (it == qs.end()) continue; it->second.tokens.push_back(kv.second.id); if (kv.second.is_end) it->second.ended = true; }
        return true;
    }
    bool RemoveQuery(int id) override { return qs.erase(id) != 0; }
    bool QueryEnded(int id) const override { auto it = qs.find(id); return it == qs.end() || it->second.ended; }
    int MaxContextLen() const override { return max_ctx; }
    SamplingStrategyId GetSamplingStrategyId(const std::string &) const override { return SamplingStrategyId::Greedy; }
    std::string Version() const override { return "loopback"; }
    std::string ModelId() const override { return "loopback"; }
    int VocabSize() const override { return vocab; }
};
}

// n_requests queries one after the other through InferFlowServiceCore::ProcessQuery over the engine above; every one must
// RETURN (a handler stuck in its wait loop is reported as "hung": the core is stopped to release it) and hand its slot back
// (an "error.busy" after max_queries earlier requests means a leak).  Writes a JSON list of the results.
int ifa_service_selftest_loop(int max_ctx, int max_queries, int fail_at_infer_call, const int *prompt, int n_prompt, int max_output_len,
                              int eos_token_id, int n_requests, int timeout_ms, char *out_json, size_t cap)
{
    if (!out_json || cap == 0 || n_prompt < 0 || (n_prompt > 0 && !prompt) || n_requests < 1) return -1;
    LoopbackEngine eng(max_ctx, max_queries, fail_at_infer_call);
    InferFlowServiceCore core(eng);
    core.Start();
    std::string js = "[";
    for (int r = 0; r < n_requests; r++) {
        InferFlowRequest req;
        req.prompt_token_ids.assign(prompt, prompt + n_prompt);
        req.max_output_len = max_output_len; req.eos_token_id = eos_token_id;
        InferFlowResponseChunk res;
        bool ok = false, hung = false;
        auto fut = std::async(std::launch::async, [&] { return core.ProcessQuery(res, req, nullptr); });
        if (fut.wait_for(std::chrono::milliseconds(timeout_ms)) != std::future_status::ready) { hung = true; core.Stop(); }
        ok = fut.get();
        if (hung) core.Start();
        std::string ids = "[";
        for (size_t i = 0; i < res.token_ids.size(); i++) { if (i) ids += ", "; ids += std::to_string(res.token_ids[i]); }
        std::string openai; res.ToJsonOpenAI(openai, false, "ifa-test");
        js += std::string(r ? ", " : "") + "{\"ok\": " + (ok ? "true" : "false") + ", \"hung\": " + (hung ? "true" : "false") + ", \"ret_code\": \"" + res.ret_code
            + "\", \"is_end\": " + (res.is_end ? "true" : "false") + ", \"finish_reason\": \"" + res.finish_reason + "\", \"token_ids\": " + ids + "], \"active\": "
            + std::to_string(eng.QueryCount()) + ", \"openai\": " + openai + "}";
    }
    core.Stop();
    js += "]";
    if (js.size() + 1 > cap) return -1;
    memcpy(out_json, js.c_str(), js.size() + 1);
    return 0;
}

// one request BODY through the parser and the loop over the loopback engine, the way the HTTP front handles it: writes
// {"ok", "ret_code", "chunks": [the streamed payloads' JSON ...], "final": the final message}.  0, or -1 on bad arguments / a small buffer.
int ifa_service_selftest_request(const char *body, int is_openai_mode, int max_ctx, char *out_json, size_t cap)
{
    if (!body || !out_json || cap == 0) return -1;
    InferFlowRequest req;
    std::string perr, js;
    if (!InferFlowServiceCore::ParseRequest(req, body, is_openai_mode != 0, &perr)) js = "{\"ok\": false, \"ret_code\": \"" + perr + "\", \"chunks\": [], \"final\": null}";
    else {
        LoopbackEngine eng(max_ctx, 4, 0);
        InferFlowServiceCore core(eng);
        core.Start();
        std::string chunks;
        std::function<bool(const InferFlowResponseChunk &)> on_chunk = [&](const InferFlowResponseChunk &c) {
            std::string one;
            if (is_openai_mode) c.ToJsonOpenAI(one, true, "ifa-test");
            else { InferFlowResponseChunk cc = c; cc.ret_code = c.is_end ? "succ" : ""; cc.time_cost = 0; cc.ToJson(one); }
            chunks += (chunks.empty() ? "" : ", ") + one;
            return true;
        };
        InferFlowResponseChunk res;
        const bool ok = core.ProcessQuery(res, req, req.is_streaming_mode ? &on_chunk : nullptr);
        core.Stop();
        res.time_cost = 0;
        std::string fin;
        if (is_openai_mode) res.ToJsonOpenAI(fin, false, "ifa-test"); else res.ToJson(fin);
        js = std::string("{\"ok\": ") + (ok ? "true" : "false") + ", \"ret_code\": \"" + res.ret_code + "\", \"chunks\": [" + chunks + "], \"final\": " + fin + "}";
    }
    if (js.size() + 1 > cap) return -1;
    memcpy(out_json, js.c_str(), js.size() + 1);
    return 0;
}

} // extern "C"
