// prefix_cache.h -- the reuse policy of the engine's prompt prefix cache (`prefix_cache = true`), as a pure host function: which KV
// slot a new query takes and how many leading rows of its prompt it finds there.  No device calls; InferenceEngine::AddQuery acts on
// the plan (ifa_model_kv_copy when the rows sit in a busy slot), the C ABI exposes it for tests (ifa_prefix_cache_plan).
#pragma once
#include <vector>

namespace inferflow_amd {

struct PrefixSlotView {
    const int *record = nullptr;    // token ids whose K/V rows the slot holds, rows [0, record_len)
    int record_len = 0;
    bool busy = false;              // a running query owns the slot: its rows may be read (copied), never taken
    long long stamp = 0;            // last use; the free slot with the oldest one is overwritten first
};

struct PrefixPlan {
    int slot = -1;                  // the query's slot
    int src_slot = -1;              // >= 0: rows [0, reuse_len) are copied from this (busy) slot first
    int reuse_len = 0;              // leading prompt tokens that need no prefill
};

// Rules:
//  1. a slot's match = common prefix of prompt and record, capped at n_prompt - 1 (one token must run to produce logits);
//  2. best = the longest match; ties: a free slot before a busy one, then the lower index;
//  3. best match < min_tokens: no reuse; the slot is the free one with an empty record and the lowest index, else the free one
//     with the oldest stamp (lower index among equals);
//  4. best slot free: taken in place;
//  5. best slot busy: destination as in 3 (never the source: it is busy), rows copied from the best slot.
// false: bad arguments, or no free slot (the caller reports "busy" before planning).
bool PlanPrefixReuse(const std::vector<PrefixSlotView> &slots, const int *prompt, int n_prompt, int min_tokens, PrefixPlan &plan);

} // namespace inferflow_amd
