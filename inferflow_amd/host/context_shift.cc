// context_shift.cc -- see context_shift.h
#include <algorithm>

#include "context_shift.h"

namespace inferflow_amd {

bool PlanContextShift(int n_tokens, int processed, int max_ctx, int keep, ContextShiftPlan &plan)
{
    plan = ContextShiftPlan();
    if (max_ctx < 2 || n_tokens < 0 || n_tokens > max_ctx || processed < 0 || processed > n_tokens || keep < 0 || keep > max_ctx / 2) return false;
    if (n_tokens < max_ctx) return true;                  // room left: no shift
    if (processed <= keep) return true;                   // (nothing behind the kept rows is in the cache yet: nothing to drop)
    plan.shift = true; plan.keep = keep;
    plan.discard = std::max(1, (processed - keep + 1) / 2);
    return true;
}

} // namespace inferflow_amd
