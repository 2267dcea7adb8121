// inference_engine.h -- the reference's InferenceEngine surface over the MI355X decode worker.
//
// Mirrors src/transformer/inference_engine.h:32-129 (class InferenceEngine),
// inference_types.h:18-179 (InferenceConfig, QueryNextToken, InferenceResult ...) and
// model.h:72-151 (ModelSpec): same member names, same argument meaning, same error convention
// (bool / query-id returns, a message through LogError -> ifa_engine_last_error(), never throws).
// The host side is plain C++ and reaches the GPU only through the C ABI of include/inferflow_amd.h.
//
// Scope: token-id queries, one model per engine.  `devices` takes the reference's grammar
// (inference_engine.cc:1738-1783): "0" one GPU; "0&1" one device group, tensor parallel (BY_TENSOR); "0;1" two groups,
// consecutive layer ranges (BY_LAYER); "0&1;2&3" HYBRID -- one worker and one host thread per GPU inside this process,
// the exchanges through the C ABI collectives (RCCL).  Tokenizers, prompt templates and the HTTP service are outside
// the hot path.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "sampling_strategy.h"

struct ifa_model;
struct ifa_comm;

namespace inferflow_amd {

struct BatchStepPlan;               // step_plan.h

struct ModelHyperParams {          // ModelHyperParams, model.h:24-70
    int vocab_size = 0, output_vocab_size = 0;
    int embd_dims = 0, hidden_dim = 0;
    int decoder_layers = 0, decoder_heads = 0, decoder_kv_heads = 0;
    int training_context_len = 0;
    int experts = 0, in_use_experts = 0, moe_top_k = 2;
    bool moe_norm_top_k_prob = true;
};

enum class TensorNormAlg { STD = 0, RMS = 1 };
enum class ActivationFn { SILU = 0, GELU = 1, RELU = 2 };
enum class PositionEmbeddingAlg { EMPTY = 0, ROPE = 1, ALIBI = 2 };

struct ModelSpec {
    std::string sid;
    bool moe_top_k_from_spec = false;      // "moe_top_k" was given in network_structure (config.json does not override it)
    ModelHyperParams hyper_params;
    std::string dir, spec_file, config_file;
    std::vector<std::string> model_files;
    std::string model_file_format;          // "llama2.c" | "safetensors" | "synthetic"
    std::string network_structure = "transformer.llama";
    TensorNormAlg norm_alg = TensorNormAlg::STD;
    ActivationFn activation_fn = ActivationFn::SILU;
    PositionEmbeddingAlg pos_embedding_alg = PositionEmbeddingAlg::ROPE;
    float rope_theta = 10000.0f, partial_rotary_factor = 1.0f, kq_scale = 1.0f;
    float attn_pre_norm_base = 0, ffn_pre_norm_base = 0, output_norm_base = 0;      // RMS weight = base + w (Gemma)
    float attn_out_scale = 1, ffn_out_scale = 1, out_scale = 1;                       // TensorOpr::Scale (MiniCPM)
    bool has_embedding_linear_norm = false;                                           // TensorOpr::LinearNorm on the decoder input (Gemma, MiniCPM)
    float embedding_linear_scale = 0;                                                 // <= 0.0001: sqrt(embd_dims)
    int qk_column_order = 0, qkv_format = 0;
    bool is_parallel_attn = false, mlp_attn_share_input = false;
    bool is_attn_post_as_residual = true;   // model.h:113: with a self_attn.post_norm, the FFN's residual is the normalised tensor
    std::string tensor_name_prefix;
    std::map<std::string, std::string> tensor_name_map;
    std::string decoding_strategy;
    // ids SamplingStrategy::GetSortedTopK never offers (sampling_strategy.cc:281-297): the vocabulary's unk id
    // (StdVocabulary::unk_id_, default 0; -1: none) and Invalid-type tokens
    int unk_token_id = 0;
    std::vector<int> invalid_token_ids;
    std::string decoder_input_template;     // kept for round-tripping the .ini; unused (token-id queries)
    int device_weight_data_type = 1;        // ElementType ids = ifa_dtype; F16
    // device_weight_data_type.<tensor> (inference_engine.cc:1664-1690; tensors attn_wq / attn_wk / attn_wv / attn_wo / ffn_w1 / ffn_w2 /
    // ffn_w3, NetworkStructure::BuildLayerTensorIdMap): per-tensor override of the type above, indexed by IFA_T_* id; -1 = Auto
    int device_weight_data_types[40] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    int device_kv_cache_data_type = 8;      // Q8_B32T2 (the reference's default, model.h:137)
    int tensor_quant_threshold = 2000 * 2000;
    static const int DEFAULT_MAX_CONTEXT_LEN = 1024;
    int max_context_len = -1;
    std::vector<std::vector<int>> device_groups;
    // "synthetic" models only: N(0, synthetic_std) weights from seed 1000 + 16*layer + tensor_id
    float synthetic_std = 0.02f;
};

struct InferenceConfig {
    struct DebugOptions { bool is_study_mode = false, show_tensors = false, enable_perf_stat = true; };
    std::vector<ModelSpec> models;
    std::string data_dir;
    int max_concurrent_queries = 10;
    std::vector<std::vector<int>> device_groups;
    int encoder_cpu_layer_count = 0, decoder_cpu_layer_count = 0, cpu_threads = 8;
    std::map<std::string, std::string> prompt_templates;
    bool return_output_tensors = false;
    // extension: queries advancing by one token share ONE batched step (rows GEMM on the matrix cores, five launches per
    // layer) from this many on; below it each runs the fused single-query decode (Llama-2-7B Q4: 2 queries batched give
    // 825 aggregate tok/s against 690 for one after the other)
    int dynamic_batching_min_queries = 2;
    // extension (tests on a 1-GPU box): run a single device through the partition path -- rank thread, communicator of
    // one rank, the C-driven step with its collectives -- instead of the plain single-worker path
    bool force_partition_path = false;
    // extension: sampled queries (and greedy ones over a vocabulary with more than 3 excluded ids) take the fused / batched step
    // and receive the step's candidate pool -- the top pool_size (value, id) pairs, built on the device by ifa_topk_pool -- instead
    // of the logits row.  Applies when return_output_tensors is false, the engine is a single device and pool_size <= IFA_POOL_MAX;
    // every other case keeps the host path.  The sampler's rules, draws and generator are the same code either way.
    bool device_sampling_pool = false;
    // extension: prompt prefix cache.  The engine remembers which token ids' K/V rows every slot holds -- a running query's
    // processed tokens, a finished query's whole context -- and AddQuery starts a prompt behind the longest run of leading tokens
    // it finds there (host/prefix_cache.h): in place if that slot is free, through one device copy into a free slot if it is
    // busy (ifa_model_kv_copy).  Matches below prefix_cache_min_tokens are not worth a slot's record.  Applies to a single-device
    // engine with return_output_tensors = false (a caller of the output tensors expects one row per prompt token); elsewhere the
    // key is accepted and the cache stays off (model_info "prefix_cache" = 0).
    bool prefix_cache = false;
    int prefix_cache_min_tokens = 16;
    // extension: device sampler.  Generate() also takes sampled queries (sample.std, top_k, sample.top_p, min_p) and processed
    // queries (penalties / logit_bias; sampled or greedy): every step of the replayed graph ends in the candidate pool and the
    // draw on the device (ifa_model_decode_sampled; the rule: csrc/ifa_sample_rule.h), the query's generator state travels to the
    // device and back, and the tokens are the ones the Infer / CommitInferenceResult loop yields for the same seeded query.
    // Applies to a single-device engine with return_output_tensors = false; elsewhere the key is accepted and inert (model_info
    // "device_sampler" = 0).  Off by default: Generate then refuses such queries as before.
    bool device_sampler = false;
    // extension: lookup decoding (InferenceEngine::GenerateLookup).  Up to lookup_draft_len (1..7) draft tokens per step, the
    // continuation of the longest n-gram of lookup_ngram_max .. lookup_ngram_min tokens that ends the query's context
    // (host/lookup_draft.h).  Applies to a single-device engine with return_output_tensors = false; elsewhere the keys are accepted
    // and GenerateLookup is refused (model_info "lookup_decoding" = 0).
    int lookup_draft_len = 4, lookup_ngram_max = 3, lookup_ngram_min = 1;
    // extension: lookup decoding for the queries the device sampler covers.  GenerateLookup also takes seeded sampled queries
    // (sample.std, top_k, sample.top_p, min_p) and processed queries (sampled or greedy): a draft step ends in the verify chain on
    // the device (ifa_model_decode_draft_sampled: the rows drawn one after the other with the query's generator, a draft accepted
    // exactly where it equals the draw), so the tokens are the ones a row-by-row loop over the same logits rows draws.  Active only
    // where device_sampler and lookup decoding both are (model_info "lookup_sampled"); off by default: GenerateLookup then refuses
    // such queries as before.
    bool lookup_sampled = false;
    // extension: context shift (host/context_shift.h; DESIGN.md "Context shift").  A query whose tokens reach max_context_len does not
    // end: the engine keeps its first context_shift_keep cache rows, drops the older half of the rows behind them and moves the rest
    // down on the device (ifa_model_kv_shift: K rows re-rotated to their new positions), then goes on.  An approximation by design
    // -- rows of layers above the first were computed while the dropped tokens were still visible -- hence opt-in.  Applies to a
    // single-device engine with return_output_tensors = false; elsewhere the keys are accepted and the shift stays off (model_info
    // "context_shift" = 0).  QueryOptions::context_shift / context_keep override both per query.
    bool context_shift = false;
    int context_shift_keep = 4;
    // extension: GenerateBatch.  A round of device-fed batched steps is at most this many steps long (1..256): it bounds the steps
    // a stopped query idles in its round and the wait before the call returns; 32 steps amortise the round's one synchronisation
    // to well under 0.1 % of the round (a design choice, not a measurement).
    int batch_generate_round_steps = 32;
    DebugOptions debug;
};

struct QueryOptions {               // SamplingStrategy::QueryOptions (sampling_strategy.h:75-81)
    int strategy_id = 0;            // SamplingStrategyId: 0 Auto (the model's decoding_strategy, greedy if none), 1 sample.std,
                                    // 2 greedy (device argmax, the hot path), 3 top_k, 4 top_p, 5 fsd, 6 random_fsd, 7 min_p, 8 tfs, 9 typical, 10 mirostat
    int random_seed = 0;            // != 0: seeds the query's generator (reproducible draws)
    float temperature = 1.0f;
    int max_output_len = -1;
    // extension: -1 off; 0: the chosen token's log-probability; 1..20: also the n most probable tokens with theirs.  The softmax is
    // over the full vocabulary at temperature 1 (the perplexity tool's), whatever the sampler does with the row afterwards.
    // Single-device engines with return_output_tensors = false only: AddQuery refuses it elsewhere.
    int logprobs = -1;
    static const int MAX_LOGPROBS = 20;
    // extension: logit processors, applied on the device to the step's logits row in front of the candidate pool and the
    // log-sum-exp (csrc/ifa_logit_adjust.hip; arithmetic and order in DESIGN.md "Logit processors").  repetition_penalty: the HF
    // rule over prompt + generated ids (x > 0 ? x / r : x * r); frequency_penalty / presence_penalty: the OpenAI rule over the
    // generated ids (x - (f * count + (count > 0 ? p : 0))); logit_bias: (id, value) pairs added last, -inf bans the id.  A query
    // with any of them non-neutral is PROCESSED: its steps end in the device pool whatever device_sampling_pool says, a greedy one
    // takes the pool's best entry, logprobs are those of the processed distribution at temperature 1.  Single-device engines with
    // return_output_tensors = false only; Generate takes a processed query only with device_sampler on, GenerateLookup only with lookup_sampled on as well.
    float repetition_penalty = 1.0f, presence_penalty = 0.0f, frequency_penalty = 0.0f;
    std::vector<std::pair<int, float>> logit_bias;
    static const int MAX_LOGIT_BIAS = 1024;
    // extension: context shift for this query.  context_shift: -1 the engine's key, 0 off, 1 on (refused where the engine cannot shift);
    // context_keep: -1 the engine's context_shift_keep, else the rows kept in front of the dropped block (0 .. max_context_len / 2)
    int context_shift = -1, context_keep = -1;
    bool Processed() const { return repetition_penalty != 1.0f || presence_penalty != 0.0f || frequency_penalty != 0.0f || !logit_bias.empty(); }
};

struct QueryInferenceResult {
    int query_id = 0;
    int prefix_len = 0;
    std::vector<IdWeight> next_tokens;          // [0] = the chosen token (greedy: weight 1; sampled: its pool probability)
    std::vector<uint16_t> output_tensor;        // F16 logits [output_rows][output_cols] if return_output_tensors
    int output_rows = 0, output_cols = 0;
    // QueryOptions::logprobs >= 0: log p of next_tokens[0] and of the `logprobs` best candidates (best first; weight = log p)
    bool has_logprobs = false;
    float chosen_logprob = 0.0f;
    std::vector<IdWeight> top_logprobs;
};

struct QueryNextToken { int id = 0; bool is_end = false; };

// what a GenerateLookup call did: worker steps in all, how many of them were draft steps (ifa_model_decode_draft), draft tokens
// offered and draft tokens that equalled the step's own greedy choice, milliseconds spent inside the worker's step calls
struct LookupStats { int steps = 0, draft_steps = 0, drafted = 0, accepted = 0; float gpu_ms = 0.0f; };

// GenerateBatch: one query of the call (in: query_id, max_new_tokens, at most 8 stop_token_ids; out: new_tokens, stopped -- the
// last new token is one of the stop ids) and what the call did: rounds of device-fed batched steps (one synchronisation each), the
// steps in them, the steps queries took alone under the batching threshold, device milliseconds inside the worker's calls
struct BatchGenerateItem { int query_id = 0, max_new_tokens = 0; std::vector<int> stop_token_ids; std::vector<int> new_tokens; bool stopped = false; };
struct BatchGenerateStats { int rounds = 0, batched_steps = 0, single_steps = 0; float gpu_ms = 0.0f; };

struct InferencePerfStat { std::map<uint32_t, float> time_map; };   // key 0: the step end to end (ms); study mode: the reference's per-phase keys, (layer + 1) * 10000 + phase

struct InferenceResult {
    std::vector<QueryInferenceResult> items;
    InferencePerfStat perf_stat;
};

// What the service shell (inferflow_service.h) needs from an engine: the query-level calls of the reference's InferenceEngine
// (src/transformer/inference_engine.h:41-75) plus two facts the reference's service reads off its query table -- whether a
// query has ended inside the engine (context full) and the context limit.  InferenceEngine implements it; the CPU tests drive
// the service loop over a host-only implementation.
class QueryEngine {
public:
    virtual ~QueryEngine() {}
    virtual int AddQuery(const std::vector<int> &tokens, const QueryOptions &query_options) = 0;
    virtual int QueryCount() const = 0;
    virtual bool Infer(InferenceResult &res) = 0;
    virtual bool CommitInferenceResult(const std::map<int, QueryNextToken> &query_map) = 0;
    virtual bool RemoveQuery(int query_id) = 0;
    virtual bool QueryEnded(int query_id) const = 0;       // true also for an unknown id
    virtual int MaxContextLen() const = 0;
    virtual SamplingStrategyId GetSamplingStrategyId(const std::string &str = "") const = 0;
    virtual std::string Version() const = 0;
    virtual std::string ModelId() const = 0;
    virtual int VocabSize() const = 0;
    // whether AddQuery accepts QueryOptions::logprobs >= 0 (the service answers "error.unsupported" otherwise)
    virtual bool SupportsLogprobs() const { return false; }
    // whether AddQuery accepts a processed query (QueryOptions::Processed(); the service answers "error.unsupported" otherwise)
    virtual bool SupportsLogitProcessors() const { return false; }
    // context shift: whether queries run past max_context_len by default (the service then does not cut max_output_len down to the
    // room behind the prompt), and whether AddQuery accepts QueryOptions::context_shift = 1 at all
    virtual bool ShiftsContext() const { return false; }
    virtual bool SupportsContextShift() const { return false; }
};

class InferenceEngine : public QueryEngine {
public:
    InferenceEngine();
    ~InferenceEngine() override;
    InferenceEngine(const InferenceEngine &) = delete;
    InferenceEngine &operator=(const InferenceEngine &) = delete;
    void Clear();

    static bool LoadConfig(InferenceConfig &config, const std::string &config_path,
                           const std::string &section, const std::string &data_root_dir = "");
    bool Init(const InferenceConfig &cfg);

    // > 0: query id, 0: busy (max_concurrent_queries reached), < 0: error
    int AddQuery(const std::vector<int> &tokens, const QueryOptions &query_options) override;
    int QueryCount() const override;
    // one step for every active query: prefill of the pending tokens, or one decode step.  A query whose context is full
    // (tokens == max_context_len) is marked ended and gets NO item (QueryEnded tells the caller) -- unless the context shift is on
    // for it: then the shift runs in front of the step and the query goes on.
    bool Infer(InferenceResult &res) override;
    bool CommitInferenceResult(const std::map<int, QueryNextToken> &query_map) override;
    bool RemoveQuery(int query_id) override;
    bool QueryEnded(int query_id) const override;
    int MaxContextLen() const override { return spec_.max_context_len > 0 ? spec_.max_context_len : ModelSpec::DEFAULT_MAX_CONTEXT_LEN; }
    std::string ModelId() const override { return spec_.sid; }
    int VocabSize() const override { return spec_.hyper_params.vocab_size; }
    bool SupportsLogprobs() const override { return model_ && !multi_ && !config_.return_output_tensors; }
    bool SupportsLogitProcessors() const override { return model_ && !multi_ && !config_.return_output_tensors; }
    bool ShiftsContext() const override { return shift_active_; }
    bool SupportsContextShift() const override { return model_ && !multi_ && !config_.return_output_tensors; }
    // context shifts so far and the tokens they dropped; the tokens query_id has dropped (-1: unknown id)
    long long context_shifts() const { return context_shifts_; }
    long long context_shift_tokens() const { return context_shift_tokens_; }
    int QueryShiftedTokens(int query_id) const;
    // Extension: a context shift with the caller's own policy (dropping one old chat turn, say): tokens [keep, keep + discard) of the
    // query and their cache rows go, the rows behind them move down.  keep >= 0, discard >= 1, keep + discard <= the query's
    // processed tokens, the query not ended; on any engine where SupportsContextShift(), whatever the context_shift key says.
    bool ShiftQuery(int query_id, int keep, int discard);
    // steps (one per query per step) whose pool was built from a row the logit processors had rewritten
    long long processed_steps() const { return processed_steps_; }

    // Extension: log p(tokens[i + 1] | tokens[0..i]) for i = 0 .. n - 2 (softmax over the full vocabulary, as the perplexity tool
    // takes it) through ifa_model_forward_score on a free KV slot: the rows' log-sum-exp and target logits are reduced on the
    // device, 2 * n floats come back instead of [n][vocab] halfs.  tokens.size() obeys AddQuery's limit (< max_context_len).
    // Single-device engines only.  lse_out / target_logit_out (nullable): the two floats logprobs_out[i] is the difference of.
    bool ScoreTokens(const std::vector<int> &tokens, std::vector<float> &logprobs_out, std::vector<float> *lse_out = nullptr,
                     std::vector<float> *target_logit_out = nullptr);

    // Extension: n steps with the token fed back on the device (hipGraph replay, no host round trip per token).  Equivalent to
    // n x {Infer, CommitInferenceResult(the step's token)}: greedy queries always; with InferenceConfig::device_sampler also sampled
    // (sample.std, top_k, sample.top_p, min_p) and processed queries, whose tokens are drawn on the device from the query's generator.
    bool Generate(int query_id, int n_steps, std::vector<int> &new_tokens, float *gpu_ms = nullptr);

    // Extension: Generate for a set of queries (DESIGN.md "Batched Generate").  Pending prompts are prefilled one by one as Generate
    // does (that step's token is the query's first new token); then rounds: the live queries in ascending id order run
    // k = min(batch_generate_round_steps, every query's remaining budget and room) steps in ONE worker call with one synchronisation
    // (ifa_model_decode_batch_steps: tokens chosen, tested against the stop ids and fed back on the device).  With no stop id hit every
    // query receives exactly the tokens of the Infer / CommitInferenceResult loop in which each query is committed until it has its
    // max_new_tokens; generator state, logit state and cache rows are equal as well.  A query that emits one of its stop ids ends
    // there (stopped = true); the others' tokens of that round are unchanged, the next rounds run without it.  Fewer live queries
    // than max(2, dynamic_batching_min_queries) run each through Generate's single-row path.  Everything is validated before
    // anything is touched: each query as Generate asks, plus no duplicate or unknown id, no more than 8 stop ids each, a
    // single-device engine, return_output_tensors = false, no more live queries than one fused batched step takes.
    bool GenerateBatch(std::vector<BatchGenerateItem> &items, float *gpu_ms = nullptr, BatchGenerateStats *stats = nullptr);
    bool batch_generate_active() const { return model_ && !multi_ && !config_.return_output_tensors; }
    long long batch_generate_steps() const { return batch_generate_steps_; }
    long long batch_generate_rounds() const { return batch_generate_rounds_; }

    // Extension: lookup decoding (prompt-lookup / "predicted outputs").  Up to max_new_tokens greedy tokens like Generate, but a step
    // carries the query's last token PLUS draft tokens -- the continuation of the context's last n-gram in `prediction` (nullable),
    // else in the query's own tokens -- as rows of one batched step on the query's slot (ifa_model_decode_draft); every leading
    // draft token that equals the step's own greedy choice is a token gained without a step of its own.  The tokens are the greedy
    // choices of the batched-rows arithmetic (F16 activations on the matrix cores); Generate's single-row step quantises its
    // activations to int8, so the two agree wherever the top-2 logit gap exceeds that route difference.  Same
    // conditions as Generate; single-device engines with return_output_tensors = false only (lookup_decoding_active()).
    bool GenerateLookup(int query_id, int max_new_tokens, std::vector<int> &new_tokens, const std::vector<int> *prediction = nullptr,
                        LookupStats *stats = nullptr);
    bool lookup_decoding_active() const { return model_ && !multi_ && !config_.return_output_tensors; }
    // InferenceConfig::lookup_sampled: whether GenerateLookup takes sampled / processed queries here; draft steps taken that way
    bool lookup_sampled_active() const { return config_.lookup_sampled && device_sampler_active_ && lookup_decoding_active(); }
    long long lookup_sampled_steps() const { return lookup_sampled_steps_; }
    // the 48-bit state of the query's generator (read-only: what the next draw starts from)
    bool QueryRngState(int query_id, unsigned long long *state);

    // id of a strategy name ("sample.top_p" ...); empty: the model's own decoding_strategy
    SamplingStrategyId GetSamplingStrategyId(const std::string &str = "") const override;
    const ModelSpec &model_spec() const { return spec_; }
    std::string Version() const override { return "inferflow_amd 0.1 (MI355X)"; }
    const InferenceConfig &config() const { return config_; }
    // "0 (E2E)\t<ms>" then "<key>\t<ms>" per line, ascending keys (InferenceEngine::PrintPerfStat, inference_engine.cc:2108-2120)
    static void PrintPerfStat(FILE *strm, const InferencePerfStat &perf_stat)
    {
        for (const auto &kv : perf_stat.time_map) {
            if (kv.first == 0) fprintf(strm, "0 (E2E)\t%g\n", kv.second);
            else fprintf(strm, "%u\t%g\n", kv.first, kv.second);
        }
    }
    int default_device_id() const { return device_; }
    int PartitionRanks() const;     // workers of the multi-GPU partition (1: single device)
    ifa_model *worker() { return model_; }
    // single-token steps of sampled queries that took the worker's decode step + device pool instead of ifa_model_forward
    // (one per query per step; 0 unless device_sampling_pool is on)
    long long sampled_fused_steps() const { return sampled_fused_steps_; }
    // device sampler (InferenceConfig::device_sampler): whether it is active on this engine; steps of Generate whose token was drawn
    // on the device
    bool device_sampler_active() const { return device_sampler_active_; }
    long long device_sampled_steps() const { return device_sampled_steps_; }
    // prompt prefix cache (InferenceConfig::prefix_cache): whether it is active on this engine; queries that started behind reused
    // rows, the rows they reused in all, how many of them needed the device copy; the rows query_id reused at AddQuery (-1: unknown id)
    bool prefix_cache_active() const { return prefix_active_; }
    long long prefix_cache_hits() const { return prefix_hits_; }
    long long prefix_cache_tokens() const { return prefix_tokens_; }
    long long prefix_cache_copies() const { return prefix_copies_; }
    int QueryCachedTokens(int query_id) const;
    // worker of partition rank r and its place in the partition (stage, n_stages, tp_rank, tp_size, layer0, layer1); rank 0 of a
    // single-device engine is worker().  The tests read the ranks' weight slices back and rebuild the whole model for the oracle.
    ifa_model *worker(int rank);
    bool WorkerPlanOf(int rank, int out6[6]) const;

private:
    struct Query {
        int id = 0;
        std::vector<int> tokens;    // committed tokens (prompt + generated)
        int processed = 0;          // tokens whose KV rows are in the cache
        QueryOptions options;
        bool ended = false;
        int kv_slot = 0;            // this query's KV cache inside the worker (ifa_model_select_kv)
        int cached_tokens = 0;      // rows the prefix cache supplied at AddQuery (processed started there)
        // context shift: on for this query, its kept rows, the tokens dropped so far.  exact_rows: cache rows [0, min(processed,
        // exact_rows)) hold exactly tokens[0 ..) at their positions -- everything until the first shift, the kept rows afterwards
        // (the moved rows were computed behind tokens that are gone: no other prompt's rows) -- what the prefix cache may record
        bool shift_on = false;
        int shift_keep = 0, shifted_tokens = 0, exact_rows = 0x7FFFFFFF;
        int counted = 0;            // a processed query: tokens[0 .. counted) are in its device logit state (the prompt, then the generated ones)
        SamplingStrategyId strategy = SamplingStrategyId::Greedy;
        StdSamplingConfig sampling; // per query copy, like StdQueryData::config
        JavaRandom rng;
        SamplingState sampling_state;   // Mirostat's mu, the FSD n-gram model, the EOS bypass count
    };
    // ---- Infer: the route of every step is planned in pure code (step_plan.h); these run the plan
    struct BatchPools { std::vector<int> ids, counts; std::vector<uint16_t> vals; std::vector<float> lse; };     // [pool_rows][pool_k]
    bool InferBatch(const std::vector<Query *> &batch, InferenceResult &res);       // the queries that advance by one token, in ONE step
    // adj_slots: empty, or per pool row of the plan the state slot of a processed query (-1: the row stays raw)
    bool BatchStep(const std::vector<int> &toks, const std::vector<int> &pos, const std::vector<int> &slots, std::vector<int> &next,
                   const BatchStepPlan &plan, const std::vector<int> &adj_slots, BatchPools &pools, std::vector<uint16_t> &all);
    bool ShiftFullQueries();        // the shift pass of Infer: every query with the shift on whose tokens have reached max_context_len
    bool ShiftIfFull(Query &q);
    bool ApplyShift(Query &q, int keep, int discard);      // device rows first, then the query's books; false: nothing changed
    int ExactRows(const Query &q) const { return std::max(0, std::min(std::min(q.processed, (int)q.tokens.size()), q.exact_rows)); }
    bool CountCommitted();          // the tokens processed queries have committed since the last step -> their device counts, one call
    bool InferQuery(Query &q, InferenceResult &res);                                // one query's own step
    bool PoolStep(Query &q, int n_new, QueryInferenceResult &item);
    bool Sampled(const Query &q) const { return q.strategy != SamplingStrategyId::Greedy || host_greedy_; }   // its token is chosen on the host
    bool EnsureLogitsRows(size_t n);                                                // logits_dev_ holds [n][vocab] halfs
    bool LogitsToHost(uint16_t *dst, size_t row0, size_t rows);
    bool SampleRow(Query &q, const uint16_t *logits_row, QueryInferenceResult &item);
    // the same from a device-built candidate pool (ifa_topk_pool: count entries of ids / F16 bits, best first)
    bool SamplePool(Query &q, const int *ids, const uint16_t *vals, int count, QueryInferenceResult &item);
    bool PoolRoute(const Query &q) const;       // this query's candidates come from the device pool (device_sampling_pool)
    int PoolLen(const Query &q) const;
    int PoolK(const Query &q) const;            // entries asked of the device: the sampler's pool length, or more for logprobs
    bool SetPoolLse(bool on);
    bool FillLogprobs(const Query &q, const int *ids, const uint16_t *vals, int count, float lse, QueryInferenceResult &item);
    // ---- Generate / GenerateLookup
    Query *FindQuery(int query_id);
    bool DeviceGreedyOk(const Query &q, int n_new, bool lookup);
    bool PrefillPending(Query &q, std::vector<int> &new_tokens, int &left, LookupStats *st);
    // device sampler: Generate draws this query's tokens on the device (a sampled strategy the device rule covers, or a processed query)
    bool DeviceDrawn(const Query &q) const;
    bool CountQuery(Query &q);                  // CountCommitted for one query
    bool PrefillPendingDrawn(Query &q, std::vector<int> &new_tokens, int &left);       // the first token from the pool step, like Infer
    bool DecodeDrawn(Query &q, int k, int *out, float *gpu_ms);
    // n_steps of Generate's single-row path behind the prefill (the loop of Generate; GenerateBatch under the batching threshold)
    bool DecodeSteps(Query &q, int n_steps, std::vector<int> &new_tokens, float &ms_total);
    long long batch_generate_steps_ = 0, batch_generate_rounds_ = 0;
    // ---- multi-GPU partitions (devices = 0&1 | 0;1 | 0&1;2&3): one worker and one host thread per GPU, like the
    // reference's Infer_TensorParallelism / Infer_Std over GpuInferenceWorker threads (inference_engine.cc:1161-1296).
    // MultiGpu and everything that looks inside it: inference_engine_multi.cc
    struct MultiGpu;
    MultiGpu *multi_ = nullptr;
    bool InitMulti(const std::vector<std::vector<int>> &groups);
    void FreeMulti();
    int LayerGroups() const;                    // device groups holding consecutive layer ranges (1: single device, or tensor parallel only)
    std::vector<ifa_model *> Workers() const;   // every rank's worker; the one worker of a single-device engine
    bool MultiBatchStep(const std::vector<int> &toks, const std::vector<int> &pos, const std::vector<int> &slots, std::vector<int> &next,
                        bool want_tensor, std::vector<uint16_t> &all);
    bool MultiStep(Query &q, int n_new, bool want_tensor, QueryInferenceResult &item, int &next);
    bool MultiDecode(const Query &q, int k, int *out, float *gpu_ms);
    InferenceConfig config_;
    ModelSpec spec_;
    ifa_model *model_ = nullptr;
    int device_ = 0;
    int next_query_id_ = 1;
    int kv_slots_ = 1;
    SamplingStrategyId default_strategy_ = SamplingStrategyId::Greedy;
    StdSamplingConfig default_sampling_;
    bool perf_phases_ = false;      // study mode: the per-phase keys of InferencePerfStat from the worker (ifa_model_perf_stat)
    bool host_greedy_ = false;      // more excluded token ids than the device argmax holds: greedy selection on the host
    std::map<int, Query> queries_;
    void *logits_dev_ = nullptr;
    size_t logits_rows_ = 0;
    long long sampled_fused_steps_ = 0, processed_steps_ = 0;
    bool device_sampler_active_ = false;       // the device_sampler key on a single-device engine without output tensors
    long long device_sampled_steps_ = 0;
    long long lookup_sampled_steps_ = 0;       // draft steps of GenerateLookup verified by the draw on the device
    bool shift_active_ = false;     // the context_shift key on an engine that can shift
    long long context_shifts_ = 0, context_shift_tokens_ = 0;
    bool pool_lse_on_ = false;      // the worker's option pool_lse as last set
    // ---- prompt prefix cache.  Record invariant: rows [0, tokens.size()) of a FREE slot's K and V hold exactly these token ids at
    // these positions.  A busy slot's record is implicit (its query's tokens[0 .. processed)); RemoveQuery turns it into the stored
    // one, and whatever else writes a free slot (ScoreTokens) clears that slot's record first.
    struct SlotRecord { std::vector<int> tokens; long long stamp = 0; };
    bool prefix_active_ = false;
    std::vector<SlotRecord> slot_records_;      // [kv_slots_] when active
    long long use_clock_ = 0;                   // stamps: a counter of record updates
    long long prefix_hits_ = 0, prefix_tokens_ = 0, prefix_copies_ = 0;
    // the new query's slot; with the cache active also q.processed / q.cached_tokens and the copy.  false: the copy failed
    bool PlaceQuery(Query &q);
};

// error text of the last failed call on this thread (the reference logs through LogError)
const char *EngineLastError();
void EngineSetError(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// the lookup_* settings are in range (engine_config.cc; LoadConfig and Init both ask)
bool LookupConfigOk(const InferenceConfig &c);
// device -> host copy on the worker's stream, then wait for it; an IFA_* code
int CopyToHostSync(ifa_model *m, void *dst, const void *src, size_t bytes);

// model loading (model_loader.cc)
bool LoadModelSpecJson(ModelSpec &spec, const std::string &path);
bool BuildWorker(ifa_model **out, ModelSpec &spec, int device);

// One worker of a multi-GPU partition (MultiGpuStrategy BY_LAYER / BY_TENSOR / HYBRID, src/transformer/model.h:61-66;
// "devices = 0&1;2&3": groups separated by ';' hold consecutive layer ranges, devices joined by '&' share every layer).
struct WorkerPlan {
    int device = 0;
    int stage = 0, n_stages = 1;        // device group (layer range) of this worker
    int tp_rank = 0, tp_size = 1;       // position inside the group
    int layer0 = 0, layer1 = -1;        // global layers [layer0, layer1); layer1 < 0: all (filled in by the loader)
    bool first_stage = true, last_stage = true;
    ifa_model *model = nullptr;
};
struct TensorSlice { size_t row0, row1, col0, col1; int local_layer; };
// the slice of tensor (layer, tid) [rows][cols] worker w holds; false: none of it
bool SliceForWorker(const WorkerPlan &w, int layer, int tid, size_t rows, size_t cols, TensorSlice &sl);
void SplitGpuLayers(int n_layers, int n_groups, std::vector<std::pair<int, int>> &ranges);
// plans: one entry per (group, rank) in the reference's device order; layer ranges are assigned from the checkpoint's layer count
bool BuildWorkers(std::vector<WorkerPlan> &plans, ModelSpec &spec);

} // namespace inferflow_amd
