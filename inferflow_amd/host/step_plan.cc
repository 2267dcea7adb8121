// step_plan.cc -- the route of an engine step (see step_plan.h).
#include <algorithm>

#include "inferflow_amd.h"
#include "step_plan.h"

namespace inferflow_amd {

QueryStepPlan PlanQueryStep(bool multi, bool return_output_tensors, bool pool_route, bool sampled, int n_new)
{
    QueryStepPlan p;
    const bool want_logits = return_output_tensors || sampled;
    if (multi) {
        p.route = StepRoute::Multi;
        if (want_logits) { p.logits_rows = n_new; p.copy = LogitsCopy::AllRows; }
    } else if (pool_route) {
        p.route = n_new == 1 ? StepRoute::DecodePool : StepRoute::ForwardPool;
        p.logits_rows = n_new == 1 ? 0 : n_new;
    } else if (n_new == 1 && !want_logits) {
        p.route = StepRoute::Decode;
    } else {
        p.route = StepRoute::Forward;
        if (want_logits) { p.logits_rows = n_new; p.copy = return_output_tensors ? LogitsCopy::AllRows : LogitsCopy::LastRow; }
    }
    return p;
}

BatchStepPlan PlanBatchStep(bool return_output_tensors, const std::vector<BatchRow> &rows)
{
    BatchStepPlan p;
    bool host_sampled = false, pinned = false;      // pinned: a row that cannot do without its pool (logprobs, logit processors)
    for (size_t r = 0; r < rows.size(); r++) {
        const BatchRow &row = rows[r];
        if (row.pool_route) {
            p.pool_rows.push_back((int)r); p.pool_k = std::max(p.pool_k, row.pool_k); p.with_lse = p.with_lse || row.wants_logprobs;
            pinned = pinned || row.wants_logprobs || row.must_pool;
        } else host_sampled = host_sampled || row.sampled;
    }
    if (host_sampled && !pinned) { p.pool_rows.clear(); p.pool_k = 0; }
    if (host_sampled && pinned) {
        for (size_t r = 0; r < rows.size(); r++) {
            const BatchRow &row = rows[r];
            if (row.pool_route || !row.sampled) continue;
            if (row.pool_len < 1 || row.pool_len > IFA_POOL_MAX) { p.error_row = (int)r; return p; }
            p.pool_rows.push_back((int)r); p.pool_k = std::max(p.pool_k, row.pool_len);
        }
        std::sort(p.pool_rows.begin(), p.pool_rows.end());
        host_sampled = false;
    }
    p.want_logits = return_output_tensors || host_sampled;
    return p;
}

GenBatchPlan PlanGenerateBatch(const GenBatchFacts &f, const std::vector<GenBatchQuery> &queries)
{
    GenBatchPlan p;
    auto refuse = [&](GenRefusal why, int id) { p = GenBatchPlan(); p.refusal = why; p.refused_id = id; return p; };
    if (f.multi_gpu) return refuse(GenRefusal::MultiGpu, 0);
    if (f.return_output_tensors) return refuse(GenRefusal::OutputTensors, 0);
    if (f.round_steps < 1 || f.round_steps > 256) return refuse(GenRefusal::BadArgument, 0);
    std::vector<const GenBatchQuery *> live;
    for (size_t i = 0; i < queries.size(); i++) {
        const GenBatchQuery &q = queries[i];
        if (q.remaining < 0 || q.room < 0) return refuse(GenRefusal::BadArgument, q.id);
        for (size_t j = 0; j < i; j++) if (queries[j].id == q.id) return refuse(GenRefusal::Duplicate, q.id);
    }
    for (const GenBatchQuery &q : queries) {
        if (q.kind != GenKind::Greedy && !f.device_sampler) return refuse(GenRefusal::NeedsSampler, q.id);
        if (!q.shift_on && q.remaining > q.room) return refuse(GenRefusal::NoRoom, q.id);
        if (q.remaining > 0) live.push_back(&q);
    }
    const bool batched = (int)live.size() >= std::max(2, f.min_queries);
    if (batched && (int)live.size() > f.fused_max) return refuse(GenRefusal::TooMany, 0);
    if (live.empty()) return p;
    std::sort(live.begin(), live.end(), [](const GenBatchQuery *a, const GenBatchQuery *b) { return a->id < b->id; });
    if (batched) {
        int k = f.round_steps;
        for (const GenBatchQuery *q : live) k = std::min(k, std::min(q->remaining, q->room));
        if (k < 1) return refuse(GenRefusal::NoRoom, live[0]->id);      // (a shift-on query at the limit with nothing to drop)
        p.route = GenRoute::Fed;
        for (const GenBatchQuery *q : live) { p.ids.push_back(q->id); p.steps.push_back(k); }
        return p;
    }
    p.route = GenRoute::Single;
    for (const GenBatchQuery *q : live) {
        int k = q->remaining;
        if (q->has_stops) k = q->kind == GenKind::Greedy ? std::min(std::min(q->remaining, q->room), f.round_steps) : 1;
        if (k < 1) return refuse(GenRefusal::NoRoom, q->id);
        p.ids.push_back(q->id); p.steps.push_back(k);
    }
    return p;
}

} // namespace inferflow_amd
