// step_plan.h -- which worker call a step of InferenceEngine::Infer takes and what it brings to the host, as pure host functions: no
// device calls, nothing of InferenceEngine.  The engine fills in the facts (PoolRoute, PoolLen, PoolK read the query and the config)
// and acts on the plan; the C ABI exposes both for tests (ifa_step_plan_query, ifa_step_plan_batch).
#pragma once
#include <vector>

namespace inferflow_amd {

enum class StepRoute { Multi = 0, DecodePool = 1, ForwardPool = 2, Decode = 3, Forward = 4 };
enum class LogitsCopy { None = 0, AllRows = 1, LastRow = 2 };

struct QueryStepPlan {
    StepRoute route = StepRoute::Forward;
    int logits_rows = 0;                    // rows the step's logits buffer must hold (0: the step writes no logits)
    LogitsCopy copy = LogitsCopy::None;     // what of them comes to the host
};

// One query's step of n_new >= 1 tokens.  pool_route: its candidates come from the device pool; sampled: its token is drawn on the host.
//  1. multi:                          Multi;       the ranks' shards of all n_new rows come over iff return_output_tensors || sampled
//  2. pool_route, n_new == 1:         DecodePool;  no logits
//  3. pool_route, n_new > 1:          ForwardPool; n_new rows stay on the device (the pool is built from the last one)
//  4. n_new == 1, no tensors, greedy: Decode;      no logits
//  5. anything else:                  Forward;     n_new rows iff return_output_tensors || sampled; AllRows for the tensors, else LastRow
QueryStepPlan PlanQueryStep(bool multi, bool return_output_tensors, bool pool_route, bool sampled, int n_new);

struct BatchRow {
    bool pool_route = false, sampled = false;
    int pool_len = 0, pool_k = 0;           // the sampler's pool length; the entries asked of the device (more for logprobs)
    bool wants_logprobs = false;
    bool must_pool = false;                 // a processed query (logit processors): its token exists only in its pool; no lse of its own
};

struct BatchStepPlan {
    std::vector<int> pool_rows;             // rows whose candidate pool is built behind the step, ascending
    int pool_k = 0;                         // one pool length serves the launch: the longest wanted (a row reads its own prefix)
    bool with_lse = false;                  // the pools come with their rows' log-sum-exp (a logprobs row is among them)
    bool want_logits = false;               // the [n][vocab] block comes to the host
    int error_row = -1;                     // >= 0: this row cannot share the step (rule 4); nothing else of the plan holds
};

// One batched decode step.  A row that is sampled and not on the pool route is "host-sampled": it needs its logits row.
//  1. pool-route rows join pool_rows; pool_k = the largest pool_k among them; with_lse: one of them wants logprobs;
//  2. a host-sampled row and no logprobs / must_pool row: the block comes over anyway, so no pools at all (pool_rows empty, pool_k 0);
//  3. a host-sampled row next to a logprobs row (which needs its pool and lse) or a must_pool row (whose pool is built from a row
//     the raw block does not show): every host-sampled row takes a pool of its pool_len
//     too -- 1 <= pool_len <= IFA_POOL_MAX, else error_row -- and no row is host-sampled any more;
//  4. want_logits = return_output_tensors || a host-sampled row is left.
BatchStepPlan PlanBatchStep(bool return_output_tensors, const std::vector<BatchRow> &rows);

// ---- InferenceEngine::GenerateBatch (DESIGN.md "Batched Generate"): the next round of a set of queries, or why the call is refused.
enum class GenKind { Greedy = 0, ProcessedGreedy = 1, Drawn = 2 };
struct GenBatchQuery {
    int id = 0;
    int remaining = 0;                      // new tokens the query still wants (0: it takes no part any more)
    int room = 0;                           // tokens it can take before max_context_len (after the shift in front of the round)
    bool shift_on = false;                  // context shift: the query goes on behind the limit, a round does not cross it
    GenKind kind = GenKind::Greedy;
    bool has_stops = false;
};
struct GenBatchFacts {
    int min_queries = 2;                    // dynamic_batching_min_queries
    int round_steps = 32;                   // batch_generate_round_steps
    int fused_max = 32;                     // rows one fused batched step takes
    bool device_sampler = false, multi_gpu = false, return_output_tensors = false;
};
enum class GenRefusal { None = 0, Duplicate = 1, MultiGpu = 2, OutputTensors = 3, TooMany = 4, NeedsSampler = 5, NoRoom = 6, BadArgument = 7 };
enum class GenRoute { Done = 0, Fed = 1, Single = 2 };
struct GenBatchPlan {
    GenRefusal refusal = GenRefusal::None;
    int refused_id = 0;                     // the query the refusal names (0: the call as a whole)
    GenRoute route = GenRoute::Done;
    std::vector<int> ids;                   // the round's queries, ascending ids (Infer's batch order)
    std::vector<int> steps;                 // per query of ids; Fed: the same number for all
};
// Refusals, in this order, nothing planned with one: a multi-GPU engine; return_output_tensors; round_steps outside 1..256 or a
// negative budget (BadArgument); an id given twice; a drawn or processed query without the device sampler; a query without the
// context shift whose budget exceeds its room; a batched round (below) of more live queries (remaining > 0) than fused_max.
// Live queries in ascending id order.  None: Done.  At least max(2, min_queries): Fed, steps = min(round_steps, min over the live
// queries of remaining and room) -- a query runs out of budget only at a round boundary, where the Infer / Commit loop loses it too.
// Fewer: Single, each live query through Generate's single-row path on its own: the whole budget without stop ids; with stop ids a
// greedy query min(remaining, room, round_steps) steps, trimmed at the stop id on the host, a processed or drawn one 1 step, so that
// generator and counts stay exact.
GenBatchPlan PlanGenerateBatch(const GenBatchFacts &facts, const std::vector<GenBatchQuery> &queries);

} // namespace inferflow_amd
