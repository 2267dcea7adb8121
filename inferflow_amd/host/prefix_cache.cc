// prefix_cache.cc -- see prefix_cache.h
#include "prefix_cache.h"

#include <algorithm>

namespace inferflow_amd {

bool PlanPrefixReuse(const std::vector<PrefixSlotView> &slots, const int *prompt, int n_prompt, int min_tokens, PrefixPlan &plan)
{
    plan = PrefixPlan();
    if (slots.empty() || !prompt || n_prompt < 1 || min_tokens < 1) return false;
    const int n = (int)slots.size();
    int fresh = -1;                 // rule 3's slot: free with an empty record, else free with the oldest stamp
    for (int i = 0; i < n; i++) {
        const PrefixSlotView &s = slots[(size_t)i];
        if (s.record_len < 0 || (s.record_len > 0 && !s.record)) return false;
        if (s.busy) continue;
        if (fresh < 0) { fresh = i; continue; }
        const PrefixSlotView &f = slots[(size_t)fresh];
        if (f.record_len == 0) continue;                            // (the lowest empty one stays)
        if (s.record_len == 0 || s.stamp < f.stamp) fresh = i;
    }
    if (fresh < 0) return false;
    int best = -1, best_len = -1;
    for (int i = 0; i < n; i++) {
        const PrefixSlotView &s = slots[(size_t)i];
        const int cap = std::min(s.record_len, n_prompt - 1);
        int len = 0;
        while (len < cap && s.record[len] == prompt[len]) len++;
        const bool better = len > best_len || (len == best_len && slots[(size_t)best].busy && !s.busy);
        if (better) { best = i; best_len = len; }
    }
    if (best_len < min_tokens) { plan.slot = fresh; return true; }
    plan.reuse_len = best_len;
    if (!slots[(size_t)best].busy) { plan.slot = best; return true; }
    plan.slot = fresh; plan.src_slot = best;
    return true;
}

} // namespace inferflow_amd
