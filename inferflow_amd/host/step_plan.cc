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

} // namespace inferflow_amd
