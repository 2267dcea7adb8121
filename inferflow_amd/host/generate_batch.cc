// generate_batch.cc -- InferenceEngine::GenerateBatch: Generate for a set of queries (DESIGN.md "Batched Generate").  The rounds are
// planned in pure code (step_plan.h, PlanGenerateBatch); a batched round is ONE worker call (ifa_model_decode_batch_steps: tokens
// chosen, tested against the stop ids and fed back on the device) with one synchronisation.
#include <algorithm>
#include <cstring>
#include <set>

#include "inferflow_amd.h"
#include "inference_engine.h"
#include "step_plan.h"

namespace inferflow_amd {

bool InferenceEngine::GenerateBatch(std::vector<BatchGenerateItem> &items, float *gpu_ms, BatchGenerateStats *stats)
{
    BatchGenerateStats st;
    for (BatchGenerateItem &it : items) { it.new_tokens.clear(); it.stopped = false; }
    if (gpu_ms) *gpu_ms = 0.0f;
    if (stats) *stats = st;
    if (!model_) { EngineSetError("The engine is not initialized"); return false; }
    // ---- everything is validated before anything is touched
    if (multi_) { EngineSetError("GenerateBatch: the device-fed batched steps run on a single-device engine (this one is a multi-GPU partition)"); return false; }
    if (config_.return_output_tensors) { EngineSetError("GenerateBatch: return_output_tensors = true asks for every step's logits on the host; use Infer / CommitInferenceResult"); return false; }
    std::vector<Query *> qs(items.size());
    std::set<int> seen;
    for (size_t i = 0; i < items.size(); i++) {
        const BatchGenerateItem &it = items[i];
        if (!seen.insert(it.query_id).second) { EngineSetError("GenerateBatch: query %d is given twice", it.query_id); return false; }
        if (!(qs[i] = FindQuery(it.query_id))) return false;
        if (it.max_new_tokens < 0) { EngineSetError("GenerateBatch: query %d: max_new_tokens %d", it.query_id, it.max_new_tokens); return false; }
        if (it.stop_token_ids.size() > IFA_BATCH_STOP_MAX) { EngineSetError("GenerateBatch: query %d has %zu stop ids, at most %d are tested on the device", it.query_id, it.stop_token_ids.size(), IFA_BATCH_STOP_MAX); return false; }
        if (!DeviceGreedyOk(*qs[i], it.max_new_tokens, false)) return false;
    }
    GenBatchFacts facts;
    facts.min_queries = config_.dynamic_batching_min_queries; facts.round_steps = config_.batch_generate_round_steps;
    facts.fused_max = ifa_model_batch_steps_rows(model_);
    facts.device_sampler = device_sampler_active_;
    const int max_ctx = MaxContextLen();
    std::vector<int> left(items.size());
    auto kind_of = [&](const Query &q) { return !DeviceDrawn(q) ? GenKind::Greedy : q.strategy == SamplingStrategyId::Greedy ? GenKind::ProcessedGreedy : GenKind::Drawn; };
    auto plan_now = [&]() {
        std::vector<GenBatchQuery> gq(items.size());
        for (size_t i = 0; i < items.size(); i++) {
            const Query &q = *qs[i];
            gq[i].id = q.id; gq[i].remaining = items[i].stopped ? 0 : left[i]; gq[i].room = std::max(0, max_ctx - (int)q.tokens.size());
            gq[i].shift_on = q.shift_on; gq[i].kind = kind_of(q); gq[i].has_stops = !items[i].stop_token_ids.empty();
        }
        return PlanGenerateBatch(facts, gq);
    };
    auto refused = [&](const GenBatchPlan &p) {
        if (p.refusal == GenRefusal::None) return false;
        const char *why = p.refusal == GenRefusal::TooMany ? "more live queries than one fused batched step of this model takes"
                        : p.refusal == GenRefusal::NoRoom ? "a query has no room left below max_context_len"
                        : p.refusal == GenRefusal::NeedsSampler ? "a sampled or processed query needs device_sampler = true"
                        : p.refusal == GenRefusal::BadArgument ? "batch_generate_round_steps outside 1..256 or a negative budget" : "refused";
        EngineSetError("GenerateBatch: %s (query %d; %zu queries, at most %d rows a step)", why, p.refused_id, items.size(), facts.fused_max);
        return true;
    };
    for (size_t i = 0; i < items.size(); i++) left[i] = items[i].max_new_tokens;
    if (refused(plan_now())) return false;
    auto is_stop = [](const BatchGenerateItem &it, int t) { return std::find(it.stop_token_ids.begin(), it.stop_token_ids.end(), t) != it.stop_token_ids.end(); };
    std::map<int, size_t> index;
    for (size_t i = 0; i < items.size(); i++) index[items[i].query_id] = i;
    // ---- pending prompts, one by one as Generate runs them (ascending ids); that step's token is the query's first new token
    for (const auto &kv : index) {
        const size_t i = kv.second;
        Query &q = *qs[i];
        if (left[i] < 1) continue;
        if (ifa_model_select_kv(model_, q.kv_slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
        if (!ShiftIfFull(q)) return false;
        if (DeviceDrawn(q) ? !PrefillPendingDrawn(q, items[i].new_tokens, left[i]) : !PrefillPending(q, items[i].new_tokens, left[i], nullptr)) return false;
        if (!items[i].new_tokens.empty() && is_stop(items[i], items[i].new_tokens.back())) items[i].stopped = true;
    }
    // ---- rounds
    for (;;) {
        for (size_t i = 0; i < items.size(); i++)
            if (!items[i].stopped && left[i] > 0 && !ShiftIfFull(*qs[i])) return false;
        const GenBatchPlan plan = plan_now();
        if (refused(plan)) return false;
        if (plan.route == GenRoute::Done) break;
        const int n = (int)plan.ids.size();
        if (plan.route == GenRoute::Single) {
            for (int r = 0; r < n; r++) {
                const size_t i = index[plan.ids[(size_t)r]];
                Query &q = *qs[i];
                BatchGenerateItem &it = items[i];
                if (ifa_model_select_kv(model_, q.kv_slot) != IFA_OK) { EngineSetError("select_kv: %s", ifa_last_error()); return false; }
                std::vector<int> out;
                float ms = 0.0f;
                if (!DecodeSteps(q, plan.steps[(size_t)r], out, ms)) return false;
                st.gpu_ms += ms; st.single_steps += (int)out.size();
                size_t keep = out.size();
                for (size_t s = 0; s < out.size(); s++)
                    if (is_stop(it, out[s])) { keep = s + 1; it.stopped = true; break; }
                // a greedy query ran on behind its stop id: those tokens never were (their cache rows lie behind `processed`)
                if (keep < out.size()) { q.tokens.resize(q.tokens.size() - (out.size() - keep)); q.processed = (int)q.tokens.size() - 1; }
                it.new_tokens.insert(it.new_tokens.end(), out.begin(), out.begin() + (long)keep);
                left[i] -= (int)keep;
            }
            continue;
        }
        const int k = plan.steps[0];
        std::vector<int> toks((size_t)n), pos((size_t)n), slots((size_t)n), out((size_t)k * (size_t)n), emitted((size_t)n);
        std::vector<ifa_batch_row> rows((size_t)n);
        for (int r = 0; r < n; r++) {
            const size_t i = index[plan.ids[(size_t)r]];
            Query &q = *qs[i];
            if (q.options.Processed() && !CountQuery(q)) return false;      // every committed token is counted before the first step reads the slot
            toks[(size_t)r] = q.tokens.back(); pos[(size_t)r] = q.processed; slots[(size_t)r] = q.kv_slot;
            ifa_batch_row &b = rows[(size_t)r];
            memset(&b, 0, sizeof(b));
            b.struct_size = (int)sizeof(b);
            const bool drawn = DeviceDrawn(q);
            b.p.strategy_id = drawn ? (int)q.strategy : (int)SamplingStrategyId::Greedy;
            b.p.temperature = q.options.temperature; b.p.top_p = q.sampling.top_p; b.p.max_k = q.sampling.max_k; b.p.min_p = q.sampling.min_p;
            b.p.pool_size = drawn ? PoolLen(q) : 1;
            b.state_slot = drawn && q.options.Processed() ? q.kv_slot : -1;
            b.rng_state = q.rng.State();
            b.n_stop = (int)items[i].stop_token_ids.size();
            for (int s = 0; s < b.n_stop; s++) b.stop_ids[s] = items[i].stop_token_ids[(size_t)s];
        }
        float ms = 0.0f;
        if (ifa_model_decode_batch_steps(model_, n, toks.data(), pos.data(), slots.data(), k, rows.data(), out.data(), emitted.data(), &ms) != IFA_OK) {
            EngineSetError("batched generate round failed: %s", ifa_last_error()); return false;
        }
        st.gpu_ms += ms; st.rounds++; st.batched_steps += k;
        batch_generate_rounds_++; batch_generate_steps_ += k;
        for (int r = 0; r < n; r++) {
            const size_t i = index[plan.ids[(size_t)r]];
            Query &q = *qs[i];
            BatchGenerateItem &it = items[i];
            const int e = emitted[(size_t)r];
            for (int s = 0; s < e; s++) { const int t = out[(size_t)s * (size_t)n + (size_t)r]; q.tokens.push_back(t); it.new_tokens.push_back(t); }
            q.processed = (int)q.tokens.size() - 1;
            left[i] -= e;
            if (DeviceDrawn(q)) {
                q.rng.SetState(rows[(size_t)r].rng_state);
                device_sampled_steps_ += e;
                if (q.options.Processed()) { processed_steps_ += e; q.counted += e; }      // (the steps counted their own tokens)
            }
            if (e > 0 && is_stop(it, it.new_tokens.back())) it.stopped = true;
            else if (e < k) { EngineSetError("GenerateBatch: query %d emitted %d of %d tokens without a stop id", q.id, e, k); return false; }
        }
    }
    if (gpu_ms) *gpu_ms = st.gpu_ms;
    if (stats) *stats = st;
    return true;
}

} // namespace inferflow_amd
