// context_shift.h -- the policy of the engine's context shift (InferenceConfig::context_shift), pure host code.
//
// A query whose tokens have reached max_context_len would end there.  With the shift on, the engine instead keeps the first `keep`
// cache rows (the attention sinks / the system prompt), drops a block of the oldest rows behind them and moves the rest down
// (ifa_model_kv_shift, csrc/ifa_kv_shift.hip) -- the "context shift" of llama.cpp, the StreamingLLM recipe.  The block is half of
// what lies behind the kept rows, as in llama.cpp, rounded UP: discard = max(1, (processed - keep + 1) / 2).  (llama.cpp rounds
// down; with an odd number of rows behind the kept ones that moves one row more than it drops.)  Rounded up, the rows that move
// never outnumber the rows that are dropped (moved = processed - keep - discard <= discard), so the device call is always one
// launch whose source and destination are disjoint.
#pragma once

namespace inferflow_amd {

struct ContextShiftPlan { bool shift = false; int keep = 0, discard = 0; };

// n_tokens: the query's committed tokens; processed: those whose rows are in the cache (0 <= processed <= n_tokens <= max_ctx);
// keep: 0 .. max_ctx / 2.  false: bad arguments.  plan.shift: the tokens have reached max_ctx and there is a row to drop.
bool PlanContextShift(int n_tokens, int processed, int max_ctx, int keep, ContextShiftPlan &plan);

} // namespace inferflow_amd
