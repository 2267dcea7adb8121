/* inferflow_engine.h -- C ABI over the C++ InferenceEngine facade (inferflow_amd/host/inference_engine.h).
 *
 * What a non-C++ caller (ctypes, cgo, JNI ...) binds to drive the reference's serving loop
 *   LoadConfig -> Init -> AddQuery -> { Infer -> CommitInferenceResult }* -> RemoveQuery
 * (InferenceEngine, src/transformer/inference_engine.h:32-129; driver loop src/tools/llm_inference.cc:345-457).
 * Return conventions are the reference's: 0/false = failure with the text in ifa_engine_last_error(),
 * AddQuery: > 0 query id, 0 busy, < 0 error.
 */
#ifndef INFERFLOW_ENGINE_H
#define INFERFLOW_ENGINE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ifa_engine ifa_engine;

/* InferenceEngine::LoadConfig(config_path, section, data_root_dir) + Init(); NULL on failure */
ifa_engine *ifa_engine_create(const char *ini_path, const char *section, const char *data_root_dir);
void ifa_engine_destroy(ifa_engine *e);
const char *ifa_engine_last_error(void);

/* AddQuery(tokens, QueryOptions{strategy greedy}) */
int ifa_engine_add_query(ifa_engine *e, const int *tokens, int n_tokens);
/* AddQuery with SamplingStrategy::QueryOptions: strategy_id = SamplingStrategyId (0 Auto = the model's decoding_strategy or
 * greedy, 1 sample.std, 2 greedy, 3 top_k, 4 top_p, 5 fsd, 6 random_fsd, 7 min_p, 8 tfs, 9 typical, 10 mirostat), random_seed != 0 seeds the
 * query's generator (sslib Random = the java.util.Random LCG), temperature as in SamplingStrategy::SoftMax */
int ifa_engine_add_query_ex(ifa_engine *e, const int *tokens, int n_tokens, int strategy_id, int random_seed, float temperature);
/* the same with QueryOptions::logprobs: -1 off; 0: the chosen token's log-probability; 1..20: also the n most probable tokens
 * with theirs (softmax over the full vocabulary at temperature 1).  The query's steps end in the device candidate pool of
 * max(the sampler's pool length, n, 1) entries plus the row's log-sum-exp (ifa_logsumexp_rows): log p = float(value) - lse;
 * tokens, rules and draws are those of the same query without logprobs.  Limits: a multi-device engine, or
 * return_output_tensors = true, returns -1 with a message; any other value of logprobs too. */
int ifa_engine_add_query_lp(ifa_engine *e, const int *tokens, int n_tokens, int strategy_id, int random_seed, float temperature, int logprobs);
/* AddQuery with every query option, as a struct that can grow: struct_size = sizeof(ifa_query_options) of the CALLER's header
 * (fields behind it keep their defaults; a size below the first field's end is refused).  strategy_id / random_seed / temperature /
 * logprobs as above.  Logit processors (csrc/ifa_logit_adjust.hip), applied on the device to the step's logits row in front of the
 * candidate pool and the log-sum-exp, in this order: repetition_penalty (> 0; 1 = off; the HF rule over prompt + generated ids:
 * x > 0 ? x / r : x * r), then x - (frequency_penalty * count + (count > 0 ? presence_penalty : 0)) over the generated ids (the
 * OpenAI rule; 0 = off), then + logit_bias: n_logit_bias (<= 1024) pairs (logit_bias_ids[i], logit_bias_values[i]), ids distinct and
 * inside the vocabulary, values finite or -inf (-inf bans the id).  A query with any of them non-neutral always takes the device pool
 * route (like a logprobs query); a greedy one receives the pool's best entry; its logprobs are those of the processed distribution
 * at temperature 1.  -1 with a message: a multi-device engine, return_output_tensors = true, more sampling candidates than a device
 * pool holds, a value outside the rules above.  ifa_engine_generate / _generate_lookup refuse such a query. */
typedef struct ifa_query_options {
    size_t struct_size;
    int strategy_id, random_seed;
    float temperature;
    int logprobs;                  /* -1 off */
    float repetition_penalty, presence_penalty, frequency_penalty;      /* 1, 0, 0 */
    int n_logit_bias;
    const int *logit_bias_ids;
    const float *logit_bias_values;
    /* context shift for this query (see ifa_engine_shift_query below).  context_shift: -1 the engine's `context_shift` key, 0 off,
     * 1 on (-1 with a message where "context_shift_available" is 0); context_keep: -1 the engine's `context_shift_keep`, else the cache
     * rows kept in front of the dropped block, 0 .. max_context_len / 2 (more is refused with a message) */
    int context_shift, context_keep;   /* -1, -1 */
} ifa_query_options;
int ifa_engine_add_query_opt(ifa_engine *e, const int *tokens, int n_tokens, const ifa_query_options *options);
/* logprobs of the query's most recent step (after ifa_engine_infer): *chosen = log p of the token the step chose; ids / logprobs
 * [min(cap, *n)] = the *n most probable tokens, best first.  1 ok, 0 failure (unknown id, or a query without logprobs). */
int ifa_engine_last_logprobs(ifa_engine *e, int query_id, float *chosen, int *ids, float *logprobs, int cap, int *n);
/* InferenceEngine::ScoreTokens: logprobs_out[i] = log p(tokens[i + 1] | tokens[0..i]) for i = 0 .. n_tokens - 2, reduced on the
 * device (ifa_model_forward_score on a free KV slot; n_tokens < max_context_len; single-device engines).  1 ok, 0 failure. */
int ifa_engine_score(ifa_engine *e, const int *tokens, int n_tokens, float *logprobs_out);
/* GetSamplingStrategyId(name): "sample.top_p", "greedy", ...; NULL/"" = the loaded model's default; 0 if unknown */
int ifa_engine_strategy_id(ifa_engine *e, const char *name);
/* host-only (no GPU): StdSamplingStrategy::ChooseTokens (src/transformer/sampling_strategy.cc:359-431) on one F16 logits
 * row, n_draws consecutive draws from a generator seeded with `seed`; writes the drawn ids / pool probabilities and the
 * pool after the top_p / max_k cut; returns the pool size or -1 */
int ifa_sampling_choose(const uint16_t *logits_f16, int vocab, int strategy_id, int max_k, float top_p, int pool_size,
                        float temperature, long long seed, int n_draws, int *out_ids, float *out_probs,
                        int *pool_ids, float *pool_probs, int pool_capacity);
/* the same for every strategy (adds 5 fsd, 6 random_fsd -- text_tokens = the query's tokens so far, consecutive draws extend the
 * n-gram model with the drawn tokens -- 7 min_p, 8 tfs, 9 typical, 10 mirostat): params9 = {max_k, top_p, pool_size, min_p, tfs z,
 * typical p, mirostat eta, mirostat tau, eos_bypassing_max}; *mirostat_mu_inout (nullable; NaN = unset -> 2 tau) carries mu across calls */
int ifa_sampling_choose_ex(const uint16_t *logits_f16, int vocab, int strategy_id, const float *params9, float temperature,
                           long long seed, int n_draws, int *out_ids, float *out_probs, int *pool_ids, float *pool_probs,
                           int pool_capacity, float *mirostat_mu_inout, const int *text_tokens, int n_text);
/* the same from a candidate pool instead of the logits row: cand_ids / cand_vals_f16 [cand_count] = the row's SortedTopK for
 * the strategy's pool length (1 for greedy, min(pool_size, vocab) otherwise), best first -- what ifa_topk_pool builds on the
 * device.  Everything else as ifa_sampling_choose_ex; given that pool it returns what ifa_sampling_choose_ex returns on the row. */
int ifa_sampling_choose_from_pool(const int *cand_ids, const uint16_t *cand_vals_f16, int cand_count, int strategy_id, const float *params9,
                                  float temperature, long long seed, int n_draws, int *out_ids, float *out_probs, int *pool_ids,
                                  float *pool_probs, int pool_capacity, float *mirostat_mu_inout, const int *text_tokens, int n_text);
/* the first n NextDouble() values of the generator seeded with `seed` (known-answer tests of the LCG) */
int ifa_sampling_random_doubles(long long seed, int n, double *out);
int ifa_engine_query_count(ifa_engine *e);
int ifa_engine_remove_query(ifa_engine *e, int query_id);           /* 1 removed, 0 unknown id */

/* Infer(): one step for every active query.  Writes up to `capacity` (query id, greedy next token) pairs and
 * returns how many were produced, or -1.  With return_output_tensors = true the F16 logits of the most recent
 * step of a query can be fetched with ifa_engine_last_logits. */
int ifa_engine_infer(ifa_engine *e, int *query_ids, int *next_tokens, int capacity);
/* CommitInferenceResult({query_id: {token, is_end}}) */
int ifa_engine_commit(ifa_engine *e, const int *query_ids, const int *tokens, const int *is_end, int n);
/* rows/cols of the logits kept from the last Infer() for this query; copies min(capacity, rows*cols) halfs */
int ifa_engine_last_logits(ifa_engine *e, int query_id, uint16_t *dst_f16, size_t capacity, int *rows, int *cols);

/* InferenceResult::perf_stat of the last Infer() (InferencePerfStat::time_map, src/transformer/inference_types.h): up to `capacity`
 * (key, milliseconds) pairs in ascending key order; returns how many keys there are.  Key 0 = the step end to end
 * (inference_engine.cc:986-988); with is_study_mode = true in the .ini also the per-phase keys (layer + 1) * 10000 + phase of
 * GpuInferenceWorker::UpdatePerfStat (inference_worker.cc:2670-2697; measured on the op-by-op step, see ifa_model_perf_stat). */
int ifa_engine_perf_stat(ifa_engine *e, unsigned *keys, float *ms, int capacity);

/* extension: n steps with device-side token feedback (graph replay); returns tokens written or -1.  Greedy, unprocessed queries
 * always.  With `device_sampler = true` in the .ini (default false; active on a single-device engine with return_output_tensors =
 * false, elsewhere accepted and inert: model_info "device_sampler" = 0) also sampled queries of sample.std / top_k / sample.top_p /
 * min_p and processed queries (penalties / logit_bias), sampled or greedy: every replayed step ends in the candidate pool and the draw
 * on the device (ifa_model_decode_sampled; the rule is pinned in csrc/ifa_sample_rule.h and DESIGN.md "Device sampler"), the query's
 * generator state goes to the device and comes back, and the tokens are exactly those of the ifa_engine_infer / ifa_engine_commit loop
 * for the same seeded query; a later infer / commit or generate continues the same generator stream.  model_info
 * "device_sampled_steps" counts the steps drawn on the device.  tfs, typical, mirostat, fsd and random_fsd queries, a vocabulary with
 * more than 3 excluded ids stay refused, and so does ifa_engine_generate_lookup unless `lookup_sampled` is on as well (below); logprobs are not produced by this call.  The device's exp is
 * ocml's (1 ulp), the host's is libm's: see the known gap in DESIGN.md.  The service shell streams through infer / commit and does not
 * use this call. */
int ifa_engine_generate(ifa_engine *e, int query_id, int n_steps, int *out_tokens, float *gpu_ms);
/* extension: ifa_engine_generate for a set of queries (DESIGN.md "Batched Generate"; model_info "batch_generate").  Query i wants up to
 * max_new[i] new tokens and ends early at one of its stop ids stop_ids[stop_offsets[i] .. stop_offsets[i + 1]) (at most 8 each;
 * stop_offsets nullable: none).  Pending prompts are prefilled one by one as ifa_engine_generate does; that step's token is the
 * query's first new token.  Then rounds: the live queries, in ascending id order, run
 *   k = min(batch_generate_round_steps (.ini, default 32, 1..256), every live query's remaining budget and room to max_context_len)
 * steps in ONE worker call with ONE synchronisation (ifa_model_decode_batch_steps: every row's token is chosen, tested against its
 * stop ids and fed back on the device); a query's context shift runs between rounds.  With no stop id hit every query receives
 * exactly the tokens of the ifa_engine_infer / ifa_engine_commit loop in which each query is committed until it has its max_new
 * tokens and then left alone; generator state, logit state and cache rows are equal as well, and infer / commit, generate or
 * another generate_batch continue any of the queries.  A query that emits a stop id ends with it (stopped[i] = 1): it stays in its
 * round as a frozen row, so the other queries' tokens of that round are unchanged, and the following rounds run without it.  A
 * round of fewer live queries than max(2, dynamic_batching_min_queries) runs each through ifa_engine_generate's single-row path.
 * out_tokens[out_offsets[i] .. +counts[i]) receives query i's tokens (out_offsets[i + 1] - out_offsets[i] >= max_new[i]);
 * stats4 (nullable): {rounds, batched steps, steps taken alone, device milliseconds}.  Returns 0, or -1 with nothing touched:
 * an unknown or repeated id, a query ifa_engine_generate would refuse (greedy always; sample.std / top_k / sample.top_p / min_p and
 * processed queries with device_sampler = true), more than 8 stop ids, a multi-GPU engine, return_output_tensors = true, more live
 * queries than one fused batched step of the model takes. */
int ifa_engine_generate_batch(ifa_engine *e, int n, const int *query_ids, const int *max_new, const int *stop_ids, const int *stop_offsets,
                              int *out_tokens, const int *out_offsets, int *counts, int *stopped, float *stats4);
/* host-only: the round rule (host/step_plan.h, PlanGenerateBatch).  facts = {dynamic_batching_min_queries, batch_generate_round_steps,
 * fused maximum, device sampler active, multi-GPU, return_output_tensors, n queries, then per query {id, remaining, room, shift on,
 * kind (0 greedy, 1 processed greedy, 2 drawn), has stop ids}}; out (at least 4 + 2 n ints) = {refusal (0 none, 1 duplicate id,
 * 2 multi-GPU, 3 output tensors, 4 too many live queries, 5 needs the device sampler, 6 no room, 7 bad argument), the id it names,
 * route (0 done, 1 device-fed batched round, 2 each query alone), m, then m x {id, steps}} in ascending id order.  0, or -1 (bad
 * arguments). */
int ifa_generate_batch_plan(const int *facts, int n_facts, int *out, int n_out);
/* extension: lookup decoding (prompt-lookup decoding / "predicted outputs").  Up to max_new greedy tokens like ifa_engine_generate,
 * but a step carries the query's last token plus up to `lookup_draft_len` (.ini, default 4, 1..7) draft tokens as rows of ONE
 * batched step on the query's KV slot (ifa_model_decode_draft); every leading draft token that equals the step's own greedy choice
 * is a token gained without a step of its own.  Drafts: the continuation of the longest n-gram (`lookup_ngram_max` .. `lookup_ngram_min`
 * tokens, defaults 3 .. 1) that ends the query's tokens, looked up in prediction[n_prediction] first (nullable / 0: none), then in
 * the query's own tokens (ifa_lookup_draft); no match: one plain step.  The tokens are the greedy choices of the batched-rows
 * arithmetic (F16 activations); ifa_engine_generate's single-row step quantises activations to int8, so the two agree wherever the
 * top-2 logit gap exceeds that route difference.  stats5 (nullable): {steps, draft steps, draft tokens offered, draft tokens
 * accepted, milliseconds inside the worker's steps}.  Returns the tokens written (never more than max_new) or -1: conditions of
 * ifa_engine_generate, and model_info "lookup_decoding" = 0 (multi-GPU engine, return_output_tensors = true).
 * With `lookup_sampled = true` in the .ini (default false; active only where "device_sampler" and "lookup_decoding" both are 1:
 * model_info "lookup_sampled") the call also takes the queries the device sampler covers -- seeded sample.std / top_k / sample.top_p /
 * min_p queries and processed queries, sampled or greedy.  A draft step then ends in the verify chain on the device
 * (ifa_model_decode_draft_sampled): the rows are drawn one after the other with the query's generator, row i + 1 counts only if
 * draft i IS the draw of row i, the chain stops at the first draw that differs.  Every draw advances the generator by exactly two
 * steps, so the tokens are exactly those a row-by-row loop over the same logits rows draws -- no rejection sampling, nothing
 * approximated -- and the generator is left where that loop leaves it (ifa_engine_query_rng_state).  A step without a draft is one
 * step of ifa_engine_generate's sampled path.  model_info "lookup_sampled_steps" counts the draft steps taken this way.  With the key
 * off such queries are refused as before; tfs, typical, mirostat, fsd and random_fsd queries and a vocabulary with more than 3
 * excluded ids stay refused either way. */
int ifa_engine_generate_lookup(ifa_engine *e, int query_id, int max_new, const int *prediction, int n_prediction, int *out_tokens,
                               float *stats5);
/* host-only: the draft rule (host/lookup_draft.h).  For g = ngram_max down to ngram_min (skipped while n_ctx < g): key = the last g
 * tokens of ctx; in pred the LOWEST start j with pred[j .. j + g) == key and j + g < n_pred gives pred[j + g ..), else in ctx the
 * HIGHEST start j < n_ctx - g with ctx[j .. j + g) == key gives ctx[j + g ..); the first g with a match wins, the draft is cut to k
 * tokens and to the end of its source.  Returns the draft length 0..k (0: no match), -1 on bad arguments. */
int ifa_lookup_draft(const int *ctx, int n_ctx, const int *pred, int n_pred, int ngram_max, int ngram_min, int k, int *draft_out);

/* the reference's perplexity harness (src/tools/perplexity.cc:41-284) over a token-id stream: windows of max_length
 * every `stride` tokens, each scored from its whole-prompt logits; needs return_output_tensors = true in the .ini and
 * no active query.  1 ok (PPL, its error estimate, scored-token count), 0 failure. */
int ifa_engine_perplexity(ifa_engine *e, const int *tokens, int n_tokens, int max_length, int stride,
                          double *ppl, double *ppl_stderr, long long *count);
/* the same harness with every window scored on the device (ifa_engine_score's path: the rows' log-sum-exp and target logits come
 * back, no [T][vocab] block): same windows, double sums and statistics.  Needs a single-device engine with
 * return_output_tensors = false in the .ini (the opposite of the call above) and no active query. */
int ifa_engine_perplexity_device(ifa_engine *e, const int *tokens, int n_tokens, int max_length, int stride,
                                 double *ppl, double *ppl_stderr, long long *count);

/* host-only: -log softmax(logits)[token_id] of one F16 logits row with the tool's arithmetic (perplexity.cc:100-119); < 0 on bad arguments */
double ifa_perplexity_token_nll(const uint16_t *logits_f16, int vocab, int token_id);

/* facts of the loaded model: "vocab_size", "embd_dims", "hidden_dim", "decoder_layers", "decoder_heads",
 * "decoder_kv_heads", "max_context_len", "device_weight_data_type", "device_kv_cache_data_type", "partition_ranks"
 * (workers of the multi-GPU partition; 1 = single device), "device_sampling_pool" (the .ini key, 0 / 1), "sampled_fused_steps"
 * (single-token steps of sampled queries served by the worker's decode step + device pool so far, one per query per step;
 * stays 0 on the host path), "prefix_cache" (0 / 1: the prompt prefix cache is ACTIVE -- the .ini key `prefix_cache = true` on a
 * single-device engine with return_output_tensors = false; elsewhere the key is accepted and this stays 0), "prefix_cache_hits"
 * (queries that started behind reused rows), "prefix_cache_tokens" (the rows they reused in all), "prefix_cache_copies" (the hits
 * whose rows sat in a busy slot and were copied on the device, ifa_model_kv_copy), "lookup_decoding" (0 / 1: ifa_engine_generate_lookup
 * is available -- a single-device engine with return_output_tensors = false), "logit_processors" (0 / 1: ifa_engine_add_query_opt accepts
 * penalties and a logit_bias -- the same condition), "processed_steps" (steps, one per query per step, whose pool was built from a
 * row the logit processors had rewritten), "context_shift" (0 / 1: queries run past max_context_len by default -- the .ini key
 * `context_shift = true` on a single-device engine with return_output_tensors = false; elsewhere the key is accepted and this stays
 * 0), "context_shift_available" (0 / 1: that condition without the key: ifa_engine_shift_query and a per-query context_shift = 1
 * work), "context_shifts" (shifts so far, automatic and explicit), "context_shift_tokens" (the tokens they dropped), "lookup_sampled" (0 / 1:
 * ifa_engine_generate_lookup takes sampled and processed queries -- the .ini key `lookup_sampled = true` where "device_sampler" and
 * "lookup_decoding" are both 1), "lookup_sampled_steps" (draft steps verified by the draw on the device); -1 if unknown */
int ifa_engine_model_info(ifa_engine *e, const char *key);
/* prompt prefix cache: the leading prompt tokens of query_id whose K/V rows AddQuery found in a slot (the query's first Infer runs
 * only the rest; QueryInferenceResult::prefix_len reports the same number); 0 without a hit or with the cache off, -1 unknown id */
int ifa_engine_query_cached_tokens(ifa_engine *e, int query_id);
/* Context shift (.ini: `context_shift = false`, `context_shift_keep = 4`; DESIGN.md "Context shift").  A query whose tokens reach
 * max_context_len is normally ended by ifa_engine_infer without an item.  With the shift on for it, the engine instead keeps its
 * first `keep` cache rows, drops the block of the oldest rows behind them and moves the rest down on the device (ifa_model_kv_shift:
 * the moved K rows are re-rotated to their new positions), erases the dropped tokens from the query and goes on; ifa_engine_generate
 * and ifa_engine_generate_lookup then accept runs that cross the limit and shift where the Infer / Commit loop would.  An
 * approximation by design: rows of layers above the first were computed while the dropped tokens were visible.  A shifted query
 * leaves only its kept rows to the prompt prefix cache; its logit processors go on counting the dropped tokens.
 * ifa_context_shift_plan (host-only) is the policy: 0 while n_tokens < max_ctx (or nothing behind `keep` is processed), else 1 with
 * out2 = {keep, discard}, discard = max(1, (processed - keep + 1) / 2) -- the older half, rounded up, so that the rows that move
 * never outnumber the dropped ones; -1: bad arguments (n_tokens > max_ctx, processed > n_tokens, keep outside 0 .. max_ctx / 2 ...).
 * ifa_engine_shift_query is the same shift with the caller's own numbers (dropping one old chat turn, say): keep >= 0, discard >= 1,
 * keep + discard <= the query's processed tokens, the query not ended, "context_shift_available" = 1; 1 ok, 0 failure with a message.
 * ifa_engine_query_shifted_tokens: the tokens query_id has dropped so far; -1 unknown id. */
int ifa_context_shift_plan(int n_tokens, int processed, int max_ctx, int keep, int *out2);
int ifa_engine_shift_query(ifa_engine *e, int query_id, int keep, int discard);
int ifa_engine_query_shifted_tokens(ifa_engine *e, int query_id);
/* read-only: the 48-bit state of query_id's generator (java.util.Random's LCG), i.e. what its next draw starts from; 1 ok, 0 unknown id */
int ifa_engine_query_rng_state(ifa_engine *e, int query_id, unsigned long long *state);
/* host-only: the cache's slot / reuse policy (host/prefix_cache.h).  Slot i holds the rows of record_lens[i] token ids -- the
 * records lie back to back in records_flat --, is busy (busy[i] != 0: a running query owns it) or free, and was last used at
 * stamps[i].  Match = common prefix of prompt and record, at most n_prompt - 1; the longest wins (ties: free before busy, then the
 * lower index).  Below min_tokens: no reuse, the slot is the lowest free one with an empty record, else the free one with the
 * oldest stamp.  Best slot free: in place.  Best slot busy: that destination + a copy.  out3 = {slot, src_slot (-1: no copy),
 * reuse_len}.  0, or -1 (bad arguments, no free slot). */
int ifa_prefix_cache_plan(const int *records_flat, const int *record_lens, const int *busy, const long long *stamps, int n_slots,
                          const int *prompt, int n_prompt, int min_tokens, int *out3);

/* host-only: the route of an engine step (host/step_plan.h), the rules ifa_engine_infer acts on.
 * query: one query's step of n_new >= 1 tokens.  multi: a multi-GPU engine; pool_route: the query's candidates come from the device
 * pool; sampled: its token is chosen on the host.  out3 = {route, logits_rows, copy}; route 0 Multi (every rank steps; the logits
 * come over iff return_output_tensors or sampled), 1 DecodePool (pool_route, n_new == 1), 2 ForwardPool (pool_route, n_new > 1:
 * n_new logits rows stay on the device), 3 Decode (n_new == 1, neither tensors nor sampled), 4 Forward (the rest: n_new logits rows
 * iff return_output_tensors or sampled); copy 0 None, 1 AllRows (return_output_tensors), 2 LastRow (sampled only).
 * batch: one batched decode step of n_rows rows, rows5[r] = {pool_route, sampled, pool_len, pool_k, wants_logprobs}.  Pool-route rows
 * get their pools, pool_k = their largest, with_lse = one of them wants logprobs.  A sampled row off the pool route needs its logits
 * row: without a logprobs row in the step it brings the whole block over and nobody gets a pool; next to one it takes a pool of its
 * pool_len instead (1 .. IFA_POOL_MAX, else error_row names it).  pool_rows_out[n_rows] receives the pool rows (ascending),
 * out5 = {number of pool rows, pool_k, with_lse, want_logits, error_row (-1: none)}.  Both: 0, or -1 (bad arguments). */
int ifa_step_plan_query(int multi, int return_output_tensors, int pool_route, int sampled, int n_new, int *out3);
int ifa_step_plan_batch(int return_output_tensors, const int *rows5, int n_rows, int *pool_rows_out, int *out5);

/* the per-device worker of partition rank `rank` (an ifa_model * for the ifa_model_* calls of inferflow_amd.h; rank 0 of a
 * single-device engine) and its place in the partition {stage, n_stages, tp_rank, tp_size, layer0, layer1}: the counterpart of
 * reaching a GpuInferenceWorker through InferenceEngine (src/transformer/inference_engine.cc:1916-1984).  NULL / -1: no such rank. */
void *ifa_engine_worker(ifa_engine *e, int rank);
int ifa_engine_worker_plan(ifa_engine *e, int rank, int *out6);

/* host-only: the partition rules the engine applies to "devices = 0&1;2&3" (BY_TENSOR slices of
 * network_builder.cc:1594-1686 / device_tensor_builder.cu:203-239, layer ranges of NetworkBuilder::SplitGpuLayers
 * :2094-2118).  slice: 1 + {row0, row1, col0, col1, local layer} of tensor (layer, tensor_id) [rows][cols] for the worker
 * at (stage, tp_rank), 0 if it holds none of it, -1 on bad arguments.  split_layers: number of groups written as
 * (start, end) pairs. */
int ifa_partition_slice(int stage, int n_stages, int tp_rank, int tp_size, int layer0, int layer1, int layer, int tensor_id,
                        size_t rows, size_t cols, size_t *out5);
int ifa_partition_split_layers(int n_layers, int n_groups, int *out_pairs, int capacity_pairs);

/* ---- service shell (host/inferflow_service.*: the token-id counterpart of src/service/inferflow_service.cc; the process is
 * bin/ifa_service <config.ini> [--port N]).  These two host-only entry points expose its request parser and response
 * formatter -- native shape and the OpenAI-shaped /chat/completions one -- so that they can be tested without a device:
 * parse writes the parsed fields back as one JSON object; both return 0, or -1 (rejected body / buffer too small). */
int ifa_service_parse_request(const char *body, int is_openai_mode, char *out_json, size_t cap);
int ifa_service_format_response(const int *token_ids, int n, int is_end, int is_openai_mode, int is_chunk, int prompt_tokens,
                                char *out_json, size_t cap);
/* host-only: the service's Infer / Commit LOOP (InferFlowServiceCore, the counterpart of src/service/inferflow_service.cc:60-129)
 * over a loopback engine with InferenceEngine's query-table semantics (a query whose context is full is ended WITHOUT an item; the
 * fail_at_infer_call-th Infer returns false).  Runs n_requests queries one after the other; writes a JSON list of
 * {ok, hung, ret_code, is_end, finish_reason, token_ids, active, openai}.  0, or -1 on bad arguments / a small buffer. */
int ifa_service_selftest_loop(int max_ctx, int max_queries, int fail_at_infer_call, const int *prompt, int n_prompt, int max_output_len,
                              int eos_token_id, int n_requests, int timeout_ms, char *out_json, size_t cap);

/* host-only: one request body through the parser and the loop over the same loopback engine (which answers a query with logprobs
 * by a fixed table: candidate j of a step is (next + j) % 1000 with log p = -0.25 - j): writes {ok, ret_code, chunks: [the streamed
 * payloads], final: the final message} with time_cost zeroed.  The body's fields are the service's: prompt_token_ids, max_output_len /
 * max_tokens, is_streaming_mode / stream, "logprobs": true, "top_logprobs": n (0..20), "repetition_penalty" (> 0), "presence_penalty" /
 * "frequency_penalty" (-2..2), "logit_bias": {"<id>": value in -100..100} (at most 300 entries) ... -- the loopback engine has no
 * logit processors: a request with them is answered "error.unsupported"; "context_shift": bool and "context_keep": int (>= 0) go to
 * the query's options -- the loopback engine cannot shift: "context_shift": true is answered "error.unsupported" */
int ifa_service_selftest_request(const char *body, int is_openai_mode, int max_ctx, char *out_json, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
