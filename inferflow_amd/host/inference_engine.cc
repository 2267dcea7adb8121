// inference_engine.cc -- InferenceEngine over the MI355X decode worker (see inference_engine.h).
// Step semantics follow InferenceEngine::Infer_Std (src/transformer/inference_engine.cc:1161-1220):
// every Infer() advances each active query by one step -- the whole pending prompt on the first
// step (prefill), one token afterwards -- and reports the candidates of the next token; the caller
// picks one and commits it with CommitInferenceResult (llm_inference.cc:345-457).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "inferflow_amd.h"
#include "inference_engine.h"
#include "step_plan.h"
#include "prefix_cache.h"
#include "lookup_draft.h"
#include "context_shift.h"
#include "half_bits.h"

namespace inferflow_amd {

InferenceEngine::InferenceEngine() {}
InferenceEngine::~InferenceEngine() { Clear(); }

void InferenceEngine::Clear()
{
    if (multi_) { FreeMulti(); model_ = nullptr; }
    if (model_) { ifa_model_destroy(model_); model_ = nullptr; }
    if (logits_dev_) { ifa_free(logits_dev_); logits_dev_ = nullptr; logits_rows_ = 0; }
    queries_.clear();
    prefix_active_ = false; slot_records_.clear();
    use_clock_ = prefix_hits_ = prefix_tokens_ = prefix_copies_ = 0;
    processed_steps_ = 0;
    shift_active_ = false; context_shifts_ = context_shift_tokens_ = 0;
    device_sampler_active_ = false; device_sampled_steps_ = 0; lookup_sampled_steps_ = 0;
}

bool InferenceEngine::Init(const InferenceConfig &cfg)
{
    Clear();
    config_ = cfg;
    if (cfg.models.empty()) { EngineSetError("No model is configured"); return false; }
    if (cfg.models.size() > 1) { EngineSetError("One model per engine (got %zu)", cfg.models.size()); return false; }
    spec_ = cfg.models[0];
    if (cfg.decoder_cpu_layer_count > 0) { EngineSetError("decoder_cpu_layer_count > 0: CPU layers are outside this engine"); return false; }
    const auto &groups = spec_.device_groups.empty() ? cfg.device_groups : spec_.device_groups;
    const bool multi = groups.size() > 1 || (!groups.empty() && groups[0].size() > 1) || cfg.force_partition_path;
    device_ = groups.empty() || groups[0].empty() ? 0 : groups[0][0];
    for (const auto &g : groups)
        for (int d : g)
            if (d < 0 || d >= ifa_device_count()) { EngineSetError("device %d is not available (%d visible)", d, ifa_device_count()); return false; }
    if (device_ < 0 || device_ >= ifa_device_count()) { EngineSetError("device %d is not available (%d visible)", device_, ifa_device_count()); return false; }
    default_strategy_ = SamplingStrategyId::Greedy; default_sampling_ = StdSamplingConfig();
    if (!spec_.decoding_strategy.empty()) {
        SamplingStrategyId sid; std::string err;
        if (!ParseDecodingStrategy(spec_.decoding_strategy, sid, default_sampling_, &err)) { EngineSetError("%s for model %s", err.c_str(), spec_.sid.c_str()); return false; }
        if (sid != SamplingStrategyId::Auto) default_strategy_ = sid;
        if (!IsSupportedStrategy(default_strategy_)) { EngineSetError("decoding_strategy \"%s\" of model %s is not supported", spec_.decoding_strategy.c_str(), spec_.sid.c_str()); return false; }
    }
    if (multi) {
        std::vector<std::vector<int>> gs = groups;
        if (gs.empty()) gs.push_back({device_});
        if (!InitMulti(gs)) { Clear(); return false; }
    } else if (!BuildWorker(&model_, spec_, device_)) return false;
    {   // the ids greedy / sampled selection never offers (GetSortedTopK): device argmax and host pool alike
        std::vector<int> excl;
        if (spec_.unk_token_id >= 0 && spec_.unk_token_id < spec_.hyper_params.vocab_size) excl.push_back(spec_.unk_token_id);
        for (int id : spec_.invalid_token_ids)
            if (id >= 0 && id < spec_.hyper_params.vocab_size && std::find(excl.begin(), excl.end(), id) == excl.end()) excl.push_back(id);
        // GetSortedTopK skips EVERY Invalid-type token: the host pool keeps the full list.  The device argmax holds three
        // ids; a vocabulary with more makes greedy queries select on the host too (one logits row per step), so that no
        // id is silently dropped
        default_sampling_.excluded_ids = excl;
        host_greedy_ = excl.size() > 3;
        if (excl.size() > 3) excl.resize(3);
        for (ifa_model *mm : Workers())
            if (ifa_model_set_excluded_tokens(mm, excl.data(), (int)excl.size()) != IFA_OK) { EngineSetError("excluded tokens: %s", ifa_last_error()); Clear(); return false; }
        // the device pool's mask has no limit: the full list
        const std::vector<int> &full = default_sampling_.excluded_ids;
        if (!multi_ && ifa_model_set_pool_excluded(model_, full.data(), (int)full.size()) != IFA_OK) {
            EngineSetError("excluded tokens of the device pool: %s", ifa_last_error()); Clear(); return false;
        }
    }
    // Per-phase keys of InferencePerfStat ((layer + 1) * 10000 + phase, inference_worker.cc:2670-2697) are filled in study mode only: the
    // reference times the host side of its launches for free, here the phases exist as separate launches only on the op-by-op step
    // (worker option perf_stat).  Key 0 (end to end) is filled whenever enable_perf_stat is on, like inference_engine.cc:986-988.
    perf_phases_ = !multi_ && config_.debug.is_study_mode && config_.debug.enable_perf_stat;
    if (perf_phases_ && ifa_model_set_option(model_, "perf_stat", 1) != IFA_OK) { EngineSetError("perf_stat: %s", ifa_last_error()); Clear(); return false; }
    // one KV cache per concurrent query, like the reference's per-query LayerKVCache sets
    kv_slots_ = std::max(1, std::min(config_.max_concurrent_queries, 64));
    for (ifa_model *mm : Workers())
        if (ifa_model_kv_slots(mm, kv_slots_) != IFA_OK) { EngineSetError("KV caches for %d queries: %s", kv_slots_, ifa_last_error()); Clear(); return false; }
    // prompt prefix cache: one device, and no caller that expects a logits row per prompt token
    if (config_.prefix_cache_min_tokens < 1) { EngineSetError("prefix_cache_min_tokens must be at least 1 (got %d)", config_.prefix_cache_min_tokens); Clear(); return false; }
    prefix_active_ = config_.prefix_cache && !multi_ && !config_.return_output_tensors;
    if (!LookupConfigOk(config_)) { Clear(); return false; }
    if (config_.context_shift_keep < 0) { EngineSetError("context_shift_keep must be at least 0 (got %d)", config_.context_shift_keep); Clear(); return false; }
    if (config_.context_shift && config_.context_shift_keep > MaxContextLen() / 2) {
        EngineSetError("context_shift_keep %d exceeds half of max_context_len %d", config_.context_shift_keep, MaxContextLen()); Clear(); return false;
    }
    shift_active_ = config_.context_shift && SupportsContextShift();
    device_sampler_active_ = config_.device_sampler && !multi_ && !config_.return_output_tensors;
    if (prefix_active_) slot_records_.assign((size_t)kv_slots_, SlotRecord());
    return true;
}

int InferenceEngine::AddQuery(const std::vector<int> &tokens, const QueryOptions &query_options)
{
    if (!model_) { EngineSetError("The engine is not initialized"); return -1; }
    if (tokens.empty()) { EngineSetError("Empty query"); return -1; }
    const int max_ctx = MaxContextLen();
    if ((int)tokens.size() >= max_ctx) { EngineSetError("The query has %zu tokens; max_context_len is %d", tokens.size(), max_ctx); return -1; }
    for (int t : tokens)
        if (t < 0 || t >= spec_.hyper_params.vocab_size) { EngineSetError("Token id %d is out of range", t); return -1; }
    SamplingStrategyId strategy = (SamplingStrategyId)query_options.strategy_id;
    if (query_options.strategy_id < 0 || query_options.strategy_id > (int)SamplingStrategyId::Mirostat) { EngineSetError("Invalid strategy id %d", query_options.strategy_id); return -1; }
    if (strategy == SamplingStrategyId::Auto) strategy = default_strategy_;
    if (!IsSupportedStrategy(strategy)) { EngineSetError("Decoding strategy %d is not supported", query_options.strategy_id); return -1; }
    if (query_options.logprobs < -1 || query_options.logprobs > QueryOptions::MAX_LOGPROBS) { EngineSetError("logprobs %d is outside -1..%d", query_options.logprobs, QueryOptions::MAX_LOGPROBS); return -1; }
    if (query_options.logprobs >= 0 && multi_) { EngineSetError("logprobs are not available on a multi-device engine (the vocabulary is sharded)"); return -1; }
    if (query_options.logprobs >= 0 && config_.return_output_tensors) { EngineSetError("logprobs are not available with return_output_tensors = true (take them from the output tensor)"); return -1; }
    const bool processed = query_options.Processed();
    if (processed && multi_) { EngineSetError("logit processors (penalties, logit_bias) are not available on a multi-device engine (the vocabulary is sharded)"); return -1; }
    if (processed && config_.return_output_tensors) { EngineSetError("logit processors (penalties, logit_bias) are not available with return_output_tensors = true (the output tensor is the raw row)"); return -1; }
    if (!(std::isfinite(query_options.repetition_penalty) && query_options.repetition_penalty > 0.0f)) { EngineSetError("repetition_penalty %g must be finite and above 0", (double)query_options.repetition_penalty); return -1; }
    if (!std::isfinite(query_options.presence_penalty) || !std::isfinite(query_options.frequency_penalty)) { EngineSetError("presence_penalty %g / frequency_penalty %g must be finite", (double)query_options.presence_penalty, (double)query_options.frequency_penalty); return -1; }
    if ((int)query_options.logit_bias.size() > QueryOptions::MAX_LOGIT_BIAS) { EngineSetError("logit_bias has %zu entries, at most %d", query_options.logit_bias.size(), QueryOptions::MAX_LOGIT_BIAS); return -1; }
    {   // every rule of the bias here, in front of the busy answer and of PlaceQuery: a refused query costs no slot record and no counter
        std::vector<int> seen;
        for (const auto &b : query_options.logit_bias) {
            if (b.first < 0 || b.first >= spec_.hyper_params.vocab_size) { EngineSetError("logit_bias id %d is outside the vocabulary", b.first); return -1; }
            if (!(std::isfinite(b.second) || b.second == -INFINITY)) { EngineSetError("logit_bias value %g for id %d must be finite or -inf", (double)b.second, b.first); return -1; }
            seen.push_back(b.first);
        }
        std::sort(seen.begin(), seen.end());
        for (size_t i = 1; i < seen.size(); i++) if (seen[i] == seen[i - 1]) { EngineSetError("logit_bias id %d is given twice", seen[i]); return -1; }
    }
    if (query_options.context_shift < -1 || query_options.context_shift > 1) { EngineSetError("context_shift %d is outside -1..1", query_options.context_shift); return -1; }
    if (query_options.context_keep < -1) { EngineSetError("context_keep %d is below -1", query_options.context_keep); return -1; }
    if (query_options.context_shift == 1 && !SupportsContextShift()) { EngineSetError("context shift is not available on a multi-device engine or with return_output_tensors = true"); return -1; }
    const bool shift_on = query_options.context_shift == -1 ? shift_active_ : query_options.context_shift == 1;
    const int shift_keep = query_options.context_keep >= 0 ? query_options.context_keep : config_.context_shift_keep;
    if (query_options.context_keep > max_ctx / 2 || (shift_on && shift_keep > max_ctx / 2)) { EngineSetError("context_keep %d exceeds half of max_context_len %d", shift_keep, max_ctx); return -1; }
    if ((int)queries_.size() >= std::min(config_.max_concurrent_queries, kv_slots_)) return 0;      // busy
    Query q; q.id = next_query_id_++; q.shift_on = shift_on; q.shift_keep = shift_keep; q.tokens = tokens; q.options = query_options;
    q.strategy = strategy; q.sampling = default_sampling_;
    if (query_options.random_seed != 0) q.rng.SetSeed((uint64_t)(int64_t)query_options.random_seed);    // SamplingStrategy::BeginQuery
    if (query_options.logprobs >= 0 && PoolK(q) > IFA_POOL_MAX) {      // (its steps could not end in a device pool: no logprobs would come back)
        EngineSetError("logprobs need the query's %d sampling candidates in one device pool of at most %d", PoolK(q), IFA_POOL_MAX); return -1;
    }
    if (processed && (PoolK(q) < 1 || PoolK(q) > IFA_POOL_MAX)) {     // (its steps could not end in a device pool: nothing would apply the processors)
        EngineSetError("logit processors need the query's %d sampling candidates in one device pool of at most %d", PoolK(q), IFA_POOL_MAX); return -1;
    }
    if (!PlaceQuery(q)) return -1;
    if (processed) {     // the WHOLE prompt, however many of its rows the prefix cache supplied: the state is about ids, not cache rows
        std::vector<int> ids; std::vector<float> vals;
        for (const auto &b : query_options.logit_bias) { ids.push_back(b.first); vals.push_back(b.second); }
        if (ifa_model_logit_state_reset(model_, q.kv_slot, q.tokens.data(), (int)q.tokens.size(), query_options.repetition_penalty, query_options.frequency_penalty,
                                        query_options.presence_penalty, ids.data(), vals.data(), (int)ids.size()) != IFA_OK) {
            EngineSetError("logit processors: %s", ifa_last_error()); return -1;
        }
        q.counted = (int)q.tokens.size();
    }
    queries_[q.id] = q;
    return q.id;
}

bool InferenceEngine::PlaceQuery(Query &q)
{
    std::vector<bool> used((size_t)kv_slots_, false);
    for (const auto &kv : queries_) used[(size_t)kv.second.kv_slot] = true;
    if (!prefix_active_) {
        while (q.kv_slot < kv_slots_ && used[(size_t)q.kv_slot]) q.kv_slot++;
        return true;
    }
    std::vector<PrefixSlotView> views((size_t)kv_slots_);
    for (int i = 0; i < kv_slots_; i++) {
        const SlotRecord &r = slot_records_[(size_t)i];
        views[(size_t)i].record = r.tokens.data(); views[(size_t)i].record_len = (int)r.tokens.size(); views[(size_t)i].stamp = r.stamp;
    }
    for (const auto &kv : queries_) {      // a running query's rows: what it has processed so far
        PrefixSlotView &v = views[(size_t)kv.second.kv_slot];
        v.busy = true; v.record = kv.second.tokens.data(); v.record_len = ExactRows(kv.second);      // (a shifted query: its kept rows only)
    }
    PrefixPlan plan;
    if (!PlanPrefixReuse(views, q.tokens.data(), (int)q.tokens.size(), config_.prefix_cache_min_tokens, plan)) {
        EngineSetError("prefix cache: no slot for query %d", q.id); return false;
    }
    // the copy runs HERE, not at the first Infer: the source query may end and its slot be overwritten in between (the worker's
    // stream orders it with the steps around it, the service serialises the engine's calls)
    if (plan.src_slot >= 0 && ifa_model_kv_copy(model_, plan.src_slot, plan.slot, plan.reuse_len) != IFA_OK) {
        EngineSetError("prefix cache: copying %d rows from slot %d to slot %d failed: %s", plan.reuse_len, plan.src_slot, plan.slot, ifa_last_error());
        slot_records_[(size_t)plan.slot] = SlotRecord();      // (whatever the destination held, it may not hold any more)
        return false;
    }
    slot_records_[(size_t)plan.slot] = SlotRecord();          // busy from here on: q.tokens[0 .. q.processed) is its record
    q.kv_slot = plan.slot; q.processed = q.cached_tokens = plan.reuse_len;
    if (plan.reuse_len > 0) { prefix_hits_++; prefix_tokens_ += plan.reuse_len; if (plan.src_slot >= 0) prefix_copies_++; }
    return true;
}

int InferenceEngine::QueryCachedTokens(int query_id) const
{
    auto it = queries_.find(query_id);
    return it == queries_.end() ? -1 : it->second.cached_tokens;
}

int InferenceEngine::QueryCount() const { return (int)queries_.size(); }
SamplingStrategyId InferenceEngine::GetSamplingStrategyId(const std::string &str) const
{
    if (str.empty()) return default_strategy_;
    return SamplingStrategyIdFromName(str);
}

// SampleTokens (inference_engine.cc:1986-2042) for the non-greedy strategies: the logits row comes to the host
bool InferenceEngine::SampleRow(Query &q, const uint16_t *logits_row, QueryInferenceResult &item)
{
    SamplingOutput out;
    if (!ChooseTokens(out, logits_row, spec_.hyper_params.vocab_size, q.strategy, q.sampling, q.options.temperature, q.rng,
                      q.sampling_state, q.tokens) || out.selected.empty()) {
        EngineSetError("Sampling failed for query %d", q.id); return false;
    }
    item.next_tokens.clear();
    item.next_tokens.push_back(out.selected[0]);
    return true;
}

bool InferenceEngine::SamplePool(Query &q, const int *ids, const uint16_t *vals, int count, QueryInferenceResult &item)
{
    std::vector<IdWeight> pool((size_t)std::max(count, 0));
    for (int i = 0; i < count; i++) { pool[(size_t)i].id = ids[i]; pool[(size_t)i].weight = HalfBitsToFloat(vals[i]); }
    SamplingOutput out;
    if (!ChooseTokensFromPool(out, std::move(pool), q.strategy, q.sampling, q.options.temperature, q.rng, q.sampling_state, q.tokens)
        || out.selected.empty()) {
        EngineSetError("Sampling failed for query %d", q.id); return false;
    }
    item.next_tokens.clear();
    item.next_tokens.push_back(out.selected[0]);
    return true;
}

int InferenceEngine::PoolLen(const Query &q) const { return PoolLength(q.strategy, q.sampling, spec_.hyper_params.vocab_size); }

int InferenceEngine::PoolK(const Query &q) const
{
    return q.options.logprobs >= 0 ? std::max(std::max(PoolLen(q), q.options.logprobs), 1) : PoolLen(q);
}

bool InferenceEngine::PoolRoute(const Query &q) const
{
    if (config_.return_output_tensors || multi_) return false;
    const int k = PoolK(q);
    if (q.options.logprobs >= 0) return k <= IFA_POOL_MAX;      // logprobs ride on the pool whatever device_sampling_pool says
    if (q.options.Processed()) return k >= 1 && k <= IFA_POOL_MAX;      // so do the logit processors: the pool is where they apply
    if (!config_.device_sampling_pool) return false;
    if (!Sampled(q)) return false;      // (the device argmax serves it)
    return k >= 1 && k <= IFA_POOL_MAX;
}

bool InferenceEngine::SetPoolLse(bool on)
{
    if (on == pool_lse_on_) return true;
    if (ifa_model_set_option(model_, "pool_lse", on ? 1 : 0) != IFA_OK) { EngineSetError("pool_lse: %s", ifa_last_error()); return false; }
    pool_lse_on_ = on;
    return true;
}

// log p = float(value) - lse for the chosen token (it must be one of the pool's) and the pool's first `logprobs` entries
bool InferenceEngine::FillLogprobs(const Query &q, const int *ids, const uint16_t *vals, int count, float lse, QueryInferenceResult &item)
{
    if (q.options.logprobs < 0) return true;
    if (item.next_tokens.empty()) { EngineSetError("logprobs: no token was chosen for query %d", q.id); return false; }
    const int chosen = item.next_tokens[0].id;
    int at = -1;
    for (int i = 0; i < count && at < 0; i++) if (ids[i] == chosen) at = i;
    if (at < 0) { EngineSetError("logprobs: the chosen token %d of query %d is not among the %d pool entries", chosen, q.id, count); return false; }
    item.has_logprobs = true;
    item.chosen_logprob = HalfBitsToFloat(vals[at]) - lse;
    item.top_logprobs.clear();
    for (int i = 0; i < std::min(count, q.options.logprobs); i++) { IdWeight w; w.id = ids[i]; w.weight = HalfBitsToFloat(vals[i]) - lse; item.top_logprobs.push_back(w); }
    return true;
}

bool InferenceEngine::ScoreTokens(const std::vector<int> &tokens, std::vector<float> &logprobs_out, std::vector<float> *lse_out,
                                  std::vector<float> *target_logit_out)
{
    logprobs_out.clear();
    if (!model_) { EngineSetError("The engine is not initialized"); return false; }
    if (multi_) { EngineSetError("ScoreTokens is not available on a multi-device engine (the vocabulary is sharded)"); return false; }
    const int n = (int)tokens.size();
    const int max_ctx = MaxContextLen();
    if (n < 2) { EngineSetError("ScoreTokens needs at least two tokens"); return false; }
    if (n >= max_ctx) { EngineSetError("ScoreTokens: %d tokens; max_context_len is %d", n, max_ctx); return false; }
    for (int t : tokens)
        if (t < 0 || t >= spec_.hyper_params.vocab_size) { EngineSetError("Token id %d is out of range", t); return false; }
    std::vector<bool> used((size_t)kv_slots_, false);
    for (const auto &kv : queries_) used[(size_t)kv.second.kv_slot] = true;
    int slot = 0;
    while (slot < kv_slots_ && used[(size_t)slot]) slot++;
    if (slot >= kv_slots_) { EngineSetError("ScoreTokens: every KV slot is taken by a query"); return false; }
    if (prefix_active_) slot_records_[(size_t)slot] = SlotRecord();      // the scoring prompt overwrites this free slot's rows
    if (ifa_model_select_kv(model_, slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
    std::vector<int> targets(tokens.begin() + 1, tokens.end());
    targets.push_back(-1);                   // (the last row scores nothing)
    std::vector<float> lse((size_t)n), tl((size_t)n);
    if (ifa_model_forward_score(model_, tokens.data(), n, 0, targets.data(), lse.data(), tl.data(), nullptr) != IFA_OK) {
        EngineSetError("scoring step failed: %s", ifa_last_error()); return false;
    }
    logprobs_out.resize((size_t)n - 1);
    for (int i = 0; i + 1 < n; i++) logprobs_out[(size_t)i] = tl[(size_t)i] - lse[(size_t)i];
    if (lse_out) lse_out->assign(lse.begin(), lse.end() - 1);
    if (target_logit_out) target_logit_out->assign(tl.begin(), tl.end() - 1);
    return true;
}

bool InferenceEngine::RemoveQuery(int query_id)
{
    auto it = queries_.find(query_id);
    if (it == queries_.end()) return false;
    if (prefix_active_) {            // the freed slot keeps the rows of the tokens the query has processed
        const Query &q = it->second;
        SlotRecord &r = slot_records_[(size_t)q.kv_slot];
        r.tokens.assign(q.tokens.begin(), q.tokens.begin() + ExactRows(q));      // (a shifted query: its kept rows only)
        r.stamp = ++use_clock_;
    }
    queries_.erase(it);
    return true;
}

bool InferenceEngine::QueryEnded(int query_id) const
{
    auto it = queries_.find(query_id);
    return it == queries_.end() || it->second.ended;
}

// ---------------------------------------------------------------------------------------------- Infer
// Infer() plans every step in pure code (step_plan.h) and runs the plan.  q.processed and the item in res.items are committed only
// after every fallible call of the step has succeeded: a query of a failed Infer() still has its tokens pending for a retry.
int CopyToHostSync(ifa_model *m, void *dst, const void *src, size_t bytes)
{
    const int rc = ifa_memcpy_d2h(dst, src, bytes, ifa_model_stream(m));
    return rc != IFA_OK ? rc : ifa_stream_sync(ifa_model_stream(m));
}

static IdWeight OneToken(int id) { IdWeight w; w.id = id; w.weight = 1.0f; return w; }      // (the device argmax chose)

bool InferenceEngine::EnsureLogitsRows(size_t n)
{
    if (n <= logits_rows_) return true;
    if (logits_dev_) ifa_free(logits_dev_);
    logits_dev_ = nullptr; logits_rows_ = 0;
    if (ifa_malloc(&logits_dev_, n * (size_t)spec_.hyper_params.vocab_size * 2) != IFA_OK) { EngineSetError("logits buffer: %s", ifa_last_error()); return false; }
    logits_rows_ = n;
    return true;
}

// rows [row0, row0 + rows) of the engine's logits buffer
bool InferenceEngine::LogitsToHost(uint16_t *dst, size_t row0, size_t rows)
{
    const size_t V = (size_t)spec_.hyper_params.vocab_size;
    if (CopyToHostSync(model_, dst, (const uint16_t *)logits_dev_ + row0 * V, rows * V * 2) != IFA_OK) { EngineSetError("logits copy: %s", ifa_last_error()); return false; }
    return true;
}

// the batched worker call of a single-device engine: the pools of plan.pool_rows and / or the [n][vocab] block come to the host
bool InferenceEngine::BatchStep(const std::vector<int> &toks, const std::vector<int> &pos, const std::vector<int> &slots, std::vector<int> &next,
                                const BatchStepPlan &plan, const std::vector<int> &adj_slots, BatchPools &pools, std::vector<uint16_t> &all)
{
    const int n = (int)toks.size();
    const size_t ns = plan.pool_rows.size();
    if (plan.want_logits && !EnsureLogitsRows((size_t)n)) return false;
    if (ns > 0) {       // no logits row leaves the device for these rows; a query reads its own prefix of the launch's sorted pool
        pools.ids.resize(ns * (size_t)plan.pool_k); pools.vals.resize(ns * (size_t)plan.pool_k); pools.counts.resize(ns);
        if (!SetPoolLse(plan.with_lse)) return false;
        if (!adj_slots.empty() && ifa_model_pool_adjust(model_, (int)ns, adj_slots.data()) != IFA_OK) { EngineSetError("logit processors: %s", ifa_last_error()); return false; }
        if (ifa_model_decode_batch_pool(model_, n, toks.data(), pos.data(), slots.data(), next.data(), plan.pool_k, plan.pool_rows.data(), (int)ns,
                                        pools.ids.data(), pools.vals.data(), pools.counts.data()) != IFA_OK) {
            EngineSetError("batched decode step failed: %s", ifa_last_error()); return false;
        }
        if (plan.with_lse) {
            pools.lse.resize(ns); int got = 0;
            if (ifa_model_pool_lse(model_, pools.lse.data(), (int)ns, &got) != IFA_OK || got != (int)ns) { EngineSetError("pool lse: %s", ifa_last_error()); return false; }
        }
        sampled_fused_steps_ += (long long)ns;
    } else if (ifa_model_decode_batch(model_, n, toks.data(), pos.data(), slots.data(), next.data(), plan.want_logits ? logits_dev_ : nullptr) != IFA_OK) {
        EngineSetError("batched decode step failed: %s", ifa_last_error()); return false;
    }
    if (plan.want_logits) all.resize((size_t)n * (size_t)spec_.hyper_params.vocab_size);
    return !plan.want_logits || LogitsToHost(all.data(), 0, (size_t)n);
}

// dynamic batching: every query that advances by exactly one token joins ONE step -- the linear layers stream the weights once
// for all of them (ifa_model_decode_batch); prefills and single queries take InferQuery
bool InferenceEngine::InferBatch(const std::vector<Query *> &batch, InferenceResult &res)
{
    const int n = (int)batch.size(), V = spec_.hyper_params.vocab_size;
    std::vector<int> toks((size_t)n), pos((size_t)n), slots((size_t)n), next((size_t)n, -1);
    std::vector<BatchRow> rows((size_t)n);
    for (int r = 0; r < n; r++) {
        const Query &q = *batch[(size_t)r];
        toks[(size_t)r] = q.tokens.back(); pos[(size_t)r] = q.processed; slots[(size_t)r] = q.kv_slot;
        BatchRow &row = rows[(size_t)r];
        // (a processed row pins the step to the pools the way a logprobs row does -- a host-sampled neighbour takes a pool of its
        //  own length instead of bringing the raw block over, which the processors never saw -- but asks for no lse)
        row.pool_route = PoolRoute(q); row.sampled = Sampled(q); row.pool_len = PoolLen(q); row.pool_k = PoolK(q);
        row.wants_logprobs = q.options.logprobs >= 0; row.must_pool = q.options.Processed();
    }
    const BatchStepPlan plan = PlanBatchStep(config_.return_output_tensors, rows);
    if (plan.error_row >= 0) {
        EngineSetError("query %d samples from %d candidates, more than a device pool holds; it cannot share a step with a logprobs or processed query",
                       batch[(size_t)plan.error_row]->id, rows[(size_t)plan.error_row].pool_len);
        return false;
    }
    BatchPools pools; std::vector<uint16_t> all;
    std::vector<int> adj_slots;
    for (size_t j = 0; j < plan.pool_rows.size(); j++) {
        const Query &q = *batch[(size_t)plan.pool_rows[j]];
        if (!q.options.Processed()) continue;
        if (adj_slots.empty()) adj_slots.assign(plan.pool_rows.size(), -1);
        adj_slots[j] = q.kv_slot;
    }
    // Query batching over a tensor-parallel device group (the reference: query batching, inference_engine.cc:1054-1124,
    // inside Infer_TensorParallelism, :1222-1296): every rank runs ONE batched step over the same queries -- merges
    // over [n][dim], one distributed argmax per row (ifa_model_tp_decode_batch) -- and hands back its vocabulary shard
    if (multi_ ? !MultiBatchStep(toks, pos, slots, next, plan.want_logits, all) : !BatchStep(toks, pos, slots, next, plan, adj_slots, pools, all)) return false;
    // the step was ONE worker call: its rows are committed together, once the item of every row is complete
    std::vector<QueryInferenceResult> items((size_t)n);
    for (int r = 0; r < n; r++) {
        Query &q = *batch[(size_t)r];
        const BatchRow &row = rows[(size_t)r];
        QueryInferenceResult &item = items[(size_t)r]; item.query_id = q.id; item.prefix_len = q.processed;
        if (!all.empty() && config_.return_output_tensors) { item.output_rows = 1; item.output_cols = V; item.output_tensor.assign(all.begin() + (size_t)r * V, all.begin() + (size_t)(r + 1) * V); }
        item.next_tokens.push_back(OneToken(next[(size_t)r]));
        const auto pr = std::find(plan.pool_rows.begin(), plan.pool_rows.end(), r);
        if (pr == plan.pool_rows.end()) {
            if (row.sampled && !SampleRow(q, all.data() + (size_t)r * V, item)) return false;
            continue;
        }
        const size_t j = (size_t)(pr - plan.pool_rows.begin());
        const int *ids = pools.ids.data() + j * (size_t)plan.pool_k; const uint16_t *vals = pools.vals.data() + j * (size_t)plan.pool_k;
        if (row.sampled && !SamplePool(q, ids, vals, std::min(pools.counts[j], row.pool_len), item)) return false;
        if (!row.sampled && q.options.Processed()) {     // the step's argmax saw the raw row: the processed greedy token is the pool's best entry
            if (pools.counts[j] < 1) { EngineSetError("logit processors left query %d no admissible token", q.id); return false; }
            item.next_tokens[0] = OneToken(ids[0]);
        }
        if (q.options.Processed()) processed_steps_++;
        if (row.wants_logprobs && !FillLogprobs(q, ids, vals, std::min(pools.counts[j], row.pool_k), pools.lse[j], item)) return false;
    }
    for (int r = 0; r < n; r++) { batch[(size_t)r]->processed = (int)batch[(size_t)r]->tokens.size(); res.items.push_back(std::move(items[(size_t)r])); }
    return true;
}

// a step that ends in the candidate pool (DecodePool / ForwardPool): nothing of size V leaves the device
bool InferenceEngine::PoolStep(Query &q, int n_new, QueryInferenceResult &item)
{
    const bool lp = q.options.logprobs >= 0;
    const bool processed = q.options.Processed();
    if (!SetPoolLse(lp)) return false;
    int ids[IFA_POOL_MAX], cnt = 0, next = -1; uint16_t vals[IFA_POOL_MAX];
    if (processed && ifa_model_pool_adjust(model_, 1, &q.kv_slot) != IFA_OK) { EngineSetError("logit processors: %s", ifa_last_error()); return false; }
    // (a prompt keeps the forward step -- lm_head over all rows into the engine's logits buffer, so its last row is bit for
    //  bit the row the host path samples from -- and only the pool of that row comes to the host)
    const int rc = n_new == 1 ? ifa_model_decode_pool(model_, q.tokens.back(), q.processed, PoolK(q), &next, ids, vals, &cnt)
                              : ifa_model_forward_pool(model_, q.tokens.data() + q.processed, n_new, q.processed, logits_dev_, PoolK(q), &next, ids, vals, &cnt);
    if (rc != IFA_OK) { EngineSetError("%s step failed: %s", n_new == 1 ? "decode" : "forward", ifa_last_error()); return false; }
    if (n_new == 1) sampled_fused_steps_++;
    if (processed) processed_steps_++;
    if (processed && !Sampled(q)) {      // the step's argmax saw the raw row: the processed greedy token is the pool's best entry
        if (cnt < 1) { EngineSetError("logit processors left query %d no admissible token", q.id); return false; }
        item.next_tokens.push_back(OneToken(ids[0]));
    } else if (!Sampled(q)) item.next_tokens.push_back(OneToken(next));
    else if (!SamplePool(q, ids, vals, std::min(cnt, PoolLen(q)), item)) return false;
    if (lp) {
        float lse = 0.0f; int got = 0;
        if (ifa_model_pool_lse(model_, &lse, 1, &got) != IFA_OK || got != 1) { EngineSetError("pool lse: %s", ifa_last_error()); return false; }
        if (!FillLogprobs(q, ids, vals, cnt, lse, item)) return false;
    }
    return true;
}

// one query's own step: the whole pending prompt, or one token outside a batch
bool InferenceEngine::InferQuery(Query &q, InferenceResult &res)
{
    const int n_new = (int)q.tokens.size() - q.processed, V = spec_.hyper_params.vocab_size;
    QueryInferenceResult item; item.query_id = q.id; item.prefix_len = q.processed;
    const bool sampled = Sampled(q);
    const QueryStepPlan plan = PlanQueryStep(multi_ != nullptr, config_.return_output_tensors, PoolRoute(q), sampled, n_new);
    int next = -1;
    if (plan.route == StepRoute::Multi) {                            // partition over several GPUs: every rank steps at once
        if (!MultiStep(q, n_new, plan.logits_rows > 0, item, next)) return false;
        if (sampled && !SampleRow(q, item.output_tensor.data() + (size_t)(n_new - 1) * V, item)) return false;
        if (!config_.return_output_tensors) { item.output_tensor.clear(); item.output_rows = item.output_cols = 0; }
    } else {
        if (ifa_model_select_kv(model_, q.kv_slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
        if (plan.logits_rows > 0 && !EnsureLogitsRows((size_t)plan.logits_rows)) return false;
        if (plan.route == StepRoute::DecodePool || plan.route == StepRoute::ForwardPool) {
            if (!PoolStep(q, n_new, item)) return false;
        } else if (plan.route == StepRoute::Decode) {                // fused graph-replayed step
            if (ifa_model_decode(model_, q.tokens.back(), q.processed, 1, &next, nullptr) != IFA_OK) { EngineSetError("decode step failed: %s", ifa_last_error()); return false; }
        } else if (ifa_model_forward(model_, q.tokens.data() + q.processed, n_new, q.processed, plan.logits_rows > 0 ? logits_dev_ : nullptr, &next) != IFA_OK) {
            EngineSetError("forward step failed: %s", ifa_last_error()); return false;
        }
        if (plan.copy != LogitsCopy::None) {                         // every row for the caller, or the last one for the host's sampler
            const bool every = plan.copy == LogitsCopy::AllRows;
            const size_t rows = every ? (size_t)n_new : 1;
            std::vector<uint16_t> last_row, &dst = every ? item.output_tensor : last_row;
            dst.resize(rows * (size_t)V);
            if (!LogitsToHost(dst.data(), (size_t)n_new - rows, rows)) return false;
            if (every) { item.output_rows = n_new; item.output_cols = V; }
            if (sampled && !SampleRow(q, dst.data() + (rows - 1) * (size_t)V, item)) return false;
        }
    }
    if (item.next_tokens.empty()) item.next_tokens.push_back(OneToken(next));
    q.processed = (int)q.tokens.size();
    res.items.push_back(std::move(item));
    return true;
}

// enqueue-only on the worker's stream, in front of this step's launches; a query's `counted` moves behind every worker call that
// has taken its pairs, so a retried Infer() does not count a token twice
bool InferenceEngine::CountCommitted()
{
    std::vector<int> slots, toks;
    std::vector<Query *> owner;
    for (auto &kv : queries_) {
        Query &q = kv.second;
        if (!q.options.Processed()) continue;
        for (int i = q.counted; i < (int)q.tokens.size(); i++) { slots.push_back(q.kv_slot); toks.push_back(q.tokens[(size_t)i]); owner.push_back(&q); }
    }
    for (size_t off = 0; off < toks.size(); off += 1024) {      // (the worker takes 1024 pairs a call; a step commits one per query)
        const size_t n = std::min<size_t>(1024, toks.size() - off);
        if (ifa_model_logit_state_add(model_, (int)n, slots.data() + off, toks.data() + off) != IFA_OK) { EngineSetError("logit processors: %s", ifa_last_error()); return false; }
        for (size_t i = off; i < off + n; i++) owner[i]->counted++;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------- context shift
int InferenceEngine::QueryShiftedTokens(int query_id) const
{
    auto it = queries_.find(query_id);
    return it == queries_.end() ? -1 : it->second.shifted_tokens;
}

// The device call is enqueue-only on the worker's stream, in front of the step's launches.  The query's device logit-processor state
// is left alone: penalties go on counting the dropped tokens (DESIGN.md "Context shift").
bool InferenceEngine::ApplyShift(Query &q, int keep, int discard)
{
    if (ifa_model_kv_shift(model_, q.kv_slot, keep, discard, q.processed) != IFA_OK) {
        EngineSetError("context shift of query %d (keep %d, discard %d, %d rows) failed: %s", q.id, keep, discard, q.processed, ifa_last_error()); return false;
    }
    q.tokens.erase(q.tokens.begin() + keep, q.tokens.begin() + keep + discard);
    q.processed -= discard;
    q.counted -= std::max(0, std::min(q.counted, keep + discard) - keep);      // the erased tokens that lay below it
    q.exact_rows = std::min(q.exact_rows, keep);
    q.shifted_tokens += discard;
    context_shifts_++; context_shift_tokens_ += discard;
    return true;
}

bool InferenceEngine::ShiftIfFull(Query &q)
{
    if (!q.shift_on || q.ended) return true;
    ContextShiftPlan plan;
    if (!PlanContextShift((int)q.tokens.size(), q.processed, MaxContextLen(), q.shift_keep, plan)) {
        EngineSetError("context shift of query %d: %zu tokens, %d processed, keep %d", q.id, q.tokens.size(), q.processed, q.shift_keep); return false;
    }
    return !plan.shift || ApplyShift(q, plan.keep, plan.discard);
}

bool InferenceEngine::ShiftFullQueries()
{
    if (multi_) return true;
    for (auto &kv : queries_) if (!ShiftIfFull(kv.second)) return false;
    return true;
}

bool InferenceEngine::ShiftQuery(int query_id, int keep, int discard)
{
    Query *qp = FindQuery(query_id);
    if (!qp) return false;
    if (!SupportsContextShift()) { EngineSetError("ShiftQuery: context shift is not available on a multi-device engine or with return_output_tensors = true"); return false; }
    if (qp->ended) { EngineSetError("ShiftQuery: query %d has ended", query_id); return false; }
    if (keep < 0 || discard < 1 || (long long)keep + discard > qp->processed) {
        EngineSetError("ShiftQuery: keep %d + discard %d of the %d processed tokens of query %d", keep, discard, qp->processed, query_id); return false;
    }
    return ApplyShift(*qp, keep, discard);
}

bool InferenceEngine::Infer(InferenceResult &res)
{
    res.items.clear(); res.perf_stat.time_map.clear();
    if (!model_) { EngineSetError("The engine is not initialized"); return false; }
    const auto t0 = std::chrono::steady_clock::now();
    const int max_ctx = MaxContextLen();
    if (!CountCommitted()) return false;
    if (!ShiftFullQueries()) return false;       // in front of the batch: the batched step and InferQuery both see the shifted query
    std::vector<Query *> batch;
    // (a partition with several layer groups steps its queries one by one: a batched step is one tensor-parallel group's)
    if (LayerGroups() == 1)
        for (auto &kv : queries_) {
            Query &q = kv.second;
            if (!q.ended && (int)q.tokens.size() < max_ctx && q.processed > 0 && (int)q.tokens.size() - q.processed == 1) batch.push_back(&q);
        }
    if ((int)batch.size() >= std::max(2, config_.dynamic_batching_min_queries) && !InferBatch(batch, res)) return false;
    for (auto &kv : queries_) {
        Query &q = kv.second;
        if (q.ended) continue;
        if ((int)q.tokens.size() >= max_ctx) { q.ended = true; continue; }
        if ((int)q.tokens.size() - q.processed <= 0) continue;       // nothing committed since the last step (or the batch took it)
        if (!InferQuery(q, res)) return false;
    }
    if (perf_phases_) {
        int keys[256]; float ms[256]; int n = 0;
        if (ifa_model_perf_stat(model_, keys, ms, 256, &n, 1) != IFA_OK) { EngineSetError("perf_stat: %s", ifa_last_error()); return false; }
        for (int i = 0; i < std::min(n, 256); i++) res.perf_stat.time_map[keys[i]] = ms[i];
    }
    if (config_.debug.enable_perf_stat)
        res.perf_stat.time_map[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return true;
}

bool InferenceEngine::CommitInferenceResult(const std::map<int, QueryNextToken> &query_map)
{
    bool ok = true;
    for (const auto &kv : query_map) {
        auto it = queries_.find(kv.first);
        if (it == queries_.end()) { EngineSetError("Query %d does not exist", kv.first); ok = false; continue; }
        Query &q = it->second;
        if (kv.second.id < 0 || kv.second.id >= spec_.hyper_params.vocab_size) { EngineSetError("Token id %d is out of range", kv.second.id); ok = false; continue; }
        q.tokens.push_back(kv.second.id);
        if (kv.second.is_end) q.ended = true;
    }
    return ok;
}

// ---------------------------------------------------------------------------------------------- Generate, GenerateLookup
InferenceEngine::Query *InferenceEngine::FindQuery(int query_id)
{
    auto it = queries_.find(query_id);
    if (!model_ || it == queries_.end()) { EngineSetError("Query %d does not exist", query_id); return nullptr; }
    return &it->second;
}

// what Generate and GenerateLookup ask of their query: not ended, greedy on the device, and the whole request fits -- nothing is
// touched unless it does (the device token ring holds 1024 steps per call)
bool InferenceEngine::DeviceGreedyOk(const Query &q, int n_new, bool lookup)
{
    if (q.ended) { EngineSetError("Query %d has ended", q.id); return false; }
    // device sampler: Generate -- and with lookup_sampled GenerateLookup -- draws on the device for the strategies its rule covers and
    // runs the processors there
    const bool sampler = lookup ? lookup_sampled_active() : device_sampler_active_;
    const bool drawn = sampler && DeviceDrawn(q);
    if (drawn && host_greedy_)
        EngineSetError(lookup ? "GenerateLookup() decodes on the device, whose argmax excludes at most 3 token ids; this vocabulary has %zu (use Infer / CommitInferenceResult)"
                              : "Generate() decodes on the device, whose argmax excludes at most 3 token ids; this vocabulary has %zu (use Infer / CommitInferenceResult)", default_sampling_.excluded_ids.size());
    else if (drawn && (PoolLen(q) < 1 || PoolLen(q) > IFA_POOL_MAX))
        EngineSetError(lookup ? "GenerateLookup() draws from a device pool of at most %d candidates; query %d asks for %d (use Infer / CommitInferenceResult)"
                              : "Generate() draws from a device pool of at most %d candidates; query %d asks for %d (use Infer / CommitInferenceResult)", IFA_POOL_MAX, q.id, PoolLen(q));
    else if (drawn) {
        if (q.shift_on || (int)q.tokens.size() + n_new <= MaxContextLen()) return true;
        EngineSetError(lookup ? "GenerateLookup: %zu tokens + %d new tokens exceed max_context_len %d" : "Generate: %zu tokens + %d steps exceed max_context_len %d", q.tokens.size(), n_new, MaxContextLen());
    } else if (sampler && q.strategy != SamplingStrategyId::Greedy)
        EngineSetError(lookup ? "GenerateLookup() draws on the device for sample.std, top_k, sample.top_p and min_p; query %d uses strategy %d (tfs, typical, mirostat, fsd and random_fsd stay with Infer / CommitInferenceResult)"
                              : "Generate() draws on the device for sample.std, top_k, sample.top_p and min_p; query %d uses strategy %d (tfs, typical, mirostat, fsd and random_fsd stay with Infer / CommitInferenceResult)", q.id, (int)q.strategy);
    else if (q.options.Processed())
        EngineSetError(lookup ? "GenerateLookup() feeds the token back on the device without logit processors; query %d has penalties or a logit_bias (use Infer / CommitInferenceResult)"
                              : "Generate() feeds the token back on the device without logit processors; query %d has penalties or a logit_bias (use Infer / CommitInferenceResult)", q.id);
    else if (host_greedy_)
        EngineSetError(lookup ? "GenerateLookup() decodes on the device, whose argmax excludes at most 3 token ids; this vocabulary has %zu (use Infer / CommitInferenceResult)"
                              : "Generate() decodes on the device, whose argmax excludes at most 3 token ids; this vocabulary has %zu (use Infer / CommitInferenceResult)", default_sampling_.excluded_ids.size());
    else if (q.strategy != SamplingStrategyId::Greedy)
        EngineSetError(lookup ? "GenerateLookup() decodes greedily on the device; query %d uses strategy %d (use Infer / CommitInferenceResult)"
                              : "Generate() decodes greedily on the device; query %d uses strategy %d (use Infer / CommitInferenceResult)", q.id, (int)q.strategy);
    else if (!q.shift_on && (int)q.tokens.size() + n_new > MaxContextLen())      // (with the context shift on the run is split at the limit)
        EngineSetError(lookup ? "GenerateLookup: %zu tokens + %d new tokens exceed max_context_len %d" : "Generate: %zu tokens + %d steps exceed max_context_len %d", q.tokens.size(), n_new, MaxContextLen());
    else return true;
    return false;
}

static float MsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// prefill whatever is pending; yields the first new token (nothing to do if only the last committed token is pending).  st: the
// step and its time are added to the lookup statistics
bool InferenceEngine::PrefillPending(Query &q, std::vector<int> &new_tokens, int &left, LookupStats *st)
{
    const int pending = (int)q.tokens.size() - q.processed;
    if (pending <= 0) { EngineSetError("Query %d has no committed token to continue from", q.id); return false; }
    if (pending == 1 && q.processed > 0) return true;
    int next = -1;
    const auto t0 = std::chrono::steady_clock::now();
    if (multi_) {
        QueryInferenceResult item;
        if (!MultiStep(q, pending, false, item, next)) return false;
    } else if (ifa_model_forward(model_, q.tokens.data() + q.processed, pending, q.processed, nullptr, &next) != IFA_OK) {
        EngineSetError("forward step failed: %s", ifa_last_error()); return false;
    }
    if (st) { st->gpu_ms += MsSince(t0); st->steps++; }
    q.processed = (int)q.tokens.size();
    q.tokens.push_back(next); new_tokens.push_back(next); left--;
    return true;
}

bool InferenceEngine::QueryRngState(int query_id, unsigned long long *state)
{
    Query *q = FindQuery(query_id);
    if (!q || !state) return false;
    *state = q->rng.State();
    return true;
}

bool InferenceEngine::DeviceDrawn(const Query &q) const
{
    if (!device_sampler_active_) return false;
    const SamplingStrategyId s = q.strategy;
    if (s == SamplingStrategyId::Greedy) return q.options.Processed();      // (an unprocessed greedy query keeps the greedy step)
    return s == SamplingStrategyId::StdSampling || s == SamplingStrategyId::TopK || s == SamplingStrategyId::TopP || s == SamplingStrategyId::MinP;
}

bool InferenceEngine::CountQuery(Query &q)
{
    while (q.counted < (int)q.tokens.size()) {
        const int n = std::min(1024, (int)q.tokens.size() - q.counted);
        const std::vector<int> slots((size_t)n, q.kv_slot);
        if (ifa_model_logit_state_add(model_, n, slots.data(), q.tokens.data() + q.counted) != IFA_OK) { EngineSetError("logit processors: %s", ifa_last_error()); return false; }
        q.counted += n;
    }
    return true;
}

// PrefillPending for a query whose tokens are drawn on the device: the pending prompt's step ends in the candidate pool and the
// host's sampler draws from it with the query's generator -- the step Infer takes, so the first token is Infer's
bool InferenceEngine::PrefillPendingDrawn(Query &q, std::vector<int> &new_tokens, int &left)
{
    const int pending = (int)q.tokens.size() - q.processed;
    if (pending <= 0) { EngineSetError("Query %d has no committed token to continue from", q.id); return false; }
    if (pending == 1 && q.processed > 0) return true;
    if (q.options.Processed() && !CountQuery(q)) return false;
    if (pending > 1 && !EnsureLogitsRows((size_t)pending)) return false;
    QueryInferenceResult item;
    if (!PoolStep(q, pending, item)) return false;
    if (item.next_tokens.empty()) { EngineSetError("Generate: the prompt step of query %d chose no token", q.id); return false; }
    const int next = item.next_tokens[0].id;
    q.processed = (int)q.tokens.size();
    q.tokens.push_back(next); new_tokens.push_back(next); left--;
    return true;
}

// k steps of the replayed graph with the draw on the device; the generator continues q.rng's stream and is handed back
bool InferenceEngine::DecodeDrawn(Query &q, int k, int *out, float *gpu_ms)
{
    const bool processed = q.options.Processed();
    if (processed && !CountQuery(q)) return false;      // every committed token is counted before the first step reads the slot
    ifa_sample_params p;
    p.strategy_id = (int)q.strategy; p.temperature = q.options.temperature; p.top_p = q.sampling.top_p; p.max_k = q.sampling.max_k;
    p.min_p = q.sampling.min_p; p.pool_size = PoolLen(q);
    unsigned long long state = q.rng.State();
    if (ifa_model_decode_sampled(model_, q.tokens.back(), q.processed, k, &p, &state, processed ? q.kv_slot : -1, out, gpu_ms) != IFA_OK) {
        EngineSetError("sampled decode failed: %s", ifa_last_error()); return false;
    }
    q.rng.SetState(state);
    device_sampled_steps_ += k;
    if (processed) { processed_steps_ += k; q.counted += k; }      // (the steps counted their own tokens; Generate appends them now)
    return true;
}

bool InferenceEngine::Generate(int query_id, int n_steps, std::vector<int> &new_tokens, float *gpu_ms)
{
    new_tokens.clear();
    Query *qp = FindQuery(query_id);
    if (!qp || n_steps <= 0) return qp != nullptr;
    Query &q = *qp;
    if (!DeviceGreedyOk(q, n_steps, false)) return false;
    if (!multi_ && ifa_model_select_kv(model_, q.kv_slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
    if (!ShiftIfFull(q)) return false;
    if (DeviceDrawn(q) ? !PrefillPendingDrawn(q, new_tokens, n_steps) : !PrefillPending(q, new_tokens, n_steps, nullptr)) return false;
    float ms_total = 0;
    if (!DecodeSteps(q, n_steps, new_tokens, ms_total)) return false;
    if (gpu_ms) *gpu_ms = ms_total;
    return true;
}

bool InferenceEngine::DecodeSteps(Query &q, int n_steps, std::vector<int> &new_tokens, float &ms_total)
{
    const bool drawn = DeviceDrawn(q);
    while (n_steps > 0) {                              // the device token ring holds 1024 steps per call
        // context shift: run to the limit, shift where Infer would (tokens == max_context_len, in front of the step), continue
        if (!ShiftIfFull(q)) return false;
        const int k = q.shift_on ? std::min(std::min(n_steps, 1024), MaxContextLen() - (int)q.tokens.size()) : std::min(n_steps, 1024);
        if (k < 1) { EngineSetError("Generate: query %d is at max_context_len %d with nothing to drop behind its %d kept rows", q.id, MaxContextLen(), q.shift_keep); return false; }
        std::vector<int> out((size_t)k);
        float ms = 0;
        if (drawn) { if (!DecodeDrawn(q, k, out.data(), &ms)) return false; }
        else if (multi_) { if (!MultiDecode(q, k, out.data(), &ms)) return false; }
        else if (ifa_model_decode(model_, q.tokens.back(), q.processed, k, out.data(), &ms) != IFA_OK) { EngineSetError("decode failed: %s", ifa_last_error()); return false; }
        ms_total += ms;
        for (int t : out) { q.tokens.push_back(t); new_tokens.push_back(t); }
        q.processed = (int)q.tokens.size() - 1;
        n_steps -= k;
    }
    return true;
}

bool InferenceEngine::GenerateLookup(int query_id, int max_new_tokens, std::vector<int> &new_tokens, const std::vector<int> *prediction,
                                     LookupStats *stats)
{
    new_tokens.clear();
    LookupStats st;
    if (stats) *stats = st;
    Query *qp = FindQuery(query_id);
    if (!qp) return false;
    if (multi_) { EngineSetError("GenerateLookup: lookup decoding runs on a single-device engine (this one has %d partition ranks)", PartitionRanks()); return false; }
    if (config_.return_output_tensors) { EngineSetError("GenerateLookup: lookup decoding is off under return_output_tensors = true (a draft step has several logits rows per step)"); return false; }
    Query &q = *qp;
    if (max_new_tokens <= 0) return true;
    if (!DeviceGreedyOk(q, max_new_tokens, true)) return false;
    if (ifa_model_select_kv(model_, q.kv_slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
    const int max_ctx = MaxContextLen();
    int left = max_new_tokens;
    if (!ShiftIfFull(q)) return false;
    // lookup_sampled: the query's tokens are drawn on the device (the queries DeviceGreedyOk has just let through)
    const bool drawn = lookup_sampled_active() && DeviceDrawn(q);
    const bool processed = drawn && q.options.Processed();
    if (drawn) {
        const size_t had = new_tokens.size();
        const auto t0 = std::chrono::steady_clock::now();
        if (!PrefillPendingDrawn(q, new_tokens, left)) return false;
        if (new_tokens.size() > had) { st.gpu_ms += MsSince(t0); st.steps++; }
    } else if (!PrefillPending(q, new_tokens, left, &st)) return false;
    ifa_sample_params sp;
    sp.strategy_id = (int)q.strategy; sp.temperature = q.options.temperature; sp.top_p = q.sampling.top_p; sp.max_k = q.sampling.max_k;
    sp.min_p = q.sampling.min_p; sp.pool_size = drawn ? PoolLen(q) : 1;
    const int *pred = prediction && !prediction->empty() ? prediction->data() : nullptr;
    const int n_pred = pred ? (int)prediction->size() : 0;
    int row[8], next[8];
    while (left > 0) {
        // here q.tokens.size() == q.processed + 1: the last token is committed, its K/V row is not in the cache yet.  A draft step
        // writes rows q.processed .. q.processed + m and may emit m + 1 tokens: m stays inside the request and the context
        // With the context shift on, the shift runs where Infer would and a draft step also leaves tokens <= max_context_len
        if (!ShiftIfFull(q)) { if (stats) *stats = st; return false; }
        if ((int)q.tokens.size() >= max_ctx) { EngineSetError("GenerateLookup: query %d is at max_context_len %d with nothing to drop behind its %d kept rows", q.id, max_ctx, q.shift_keep); if (stats) *stats = st; return false; }
        const int pos0 = q.processed;
        const int m_max = std::min(std::min(config_.lookup_draft_len, left - 1), max_ctx - pos0 - 1 - (q.shift_on ? 1 : 0));
        const int m = m_max >= 1 ? LookupDraft(q.tokens.data(), (int)q.tokens.size(), pred, n_pred, config_.lookup_ngram_max, config_.lookup_ngram_min, m_max, row + 1) : 0;
        if (m < 0) { EngineSetError("GenerateLookup: draft lookup failed"); return false; }
        st.steps++;
        if (m == 0) {                                  // nothing to guess: one plain step
            float ms = 0;
            if (drawn) { if (!DecodeDrawn(q, 1, next, &ms)) { if (stats) *stats = st; return false; } }
            else if (ifa_model_decode(model_, q.tokens.back(), pos0, 1, next, &ms) != IFA_OK) { EngineSetError("decode failed: %s", ifa_last_error()); if (stats) *stats = st; return false; }
            st.gpu_ms += ms;
            q.tokens.push_back(next[0]); new_tokens.push_back(next[0]);
            q.processed = pos0 + 1;
            left--;
            continue;
        }
        row[0] = q.tokens.back();
        const auto t0 = std::chrono::steady_clock::now();
        int a = 0;
        if (drawn) {
            // the rows drawn one after the other on the device with the query's generator: draft i is accepted exactly where it IS the
            // draw of row i - 1, so the emitted tokens are what a row-by-row loop over these logits rows draws
            if (processed && !CountQuery(q)) { if (stats) *stats = st; return false; }      // every committed token counted before the step reads the slot
            unsigned long long state = q.rng.State();
            int emitted = 0;
            if (ifa_model_decode_draft_sampled(model_, m + 1, row, pos0, &sp, &state, processed ? q.kv_slot : -1, next, &emitted) != IFA_OK) {
                EngineSetError("sampled draft step failed: %s", ifa_last_error()); if (stats) *stats = st; return false;
            }
            q.rng.SetState(state);
            a = emitted - 1;
            lookup_sampled_steps_++;
            if (processed) processed_steps_++;
        } else {
            if (ifa_model_decode_draft(model_, m + 1, row, pos0, next, nullptr) != IFA_OK) { EngineSetError("draft step failed: %s", ifa_last_error()); if (stats) *stats = st; return false; }
            while (a < m && next[a] == row[a + 1]) a++;
        }
        st.gpu_ms += MsSince(t0);
        st.draft_steps++; st.drafted += m; st.accepted += a;
        // rows pos0 .. pos0 + a hold the last token and the a accepted drafts -- the tokens in front of the newest one; the rejected
        // rows behind them lie outside tokens[0 .. processed) (the prefix cache's record) and the next step overwrites them
        for (int i = 0; i <= a; i++) { q.tokens.push_back(next[i]); new_tokens.push_back(next[i]); }
        q.processed = pos0 + a + 1;
        left -= a + 1;
        if (processed && !CountQuery(q)) { if (stats) *stats = st; return false; }      // (the draft step counts nothing itself)
    }
    if (stats) *stats = st;
    return true;
}

} // namespace inferflow_amd
