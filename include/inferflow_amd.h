/*
 * inferflow_amd.h -- C ABI of the MI355X-native quantized decode path.
 *
 * This is the drop-in boundary for the lower surface that Inferflow's
 * GpuInferenceWorker calls:
 *   TensorOpr::*      src/tensor/tensor_opr.h:33-131
 *   TensorMul::*      src/tensor/tensor_mul.h:14-57
 *   CublasEngine      src/tensor/cublas_engine.h:31-33
 *   LayerKVCache      src/transformer/kv_cache.h:13-34
 *   CudaUtil          src/common/cuda_util.h:40-61
 * and, one level up, for the per-step work of GpuInferenceWorker::Run
 * (src/transformer/inference_worker.cc:234-340) behind InferenceEngine
 * (src/transformer/inference_engine.h:32-129).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - Every function returns 0 on success or a negative IFA_ERR_* code;
 *    ifa_last_error() returns the message of the last failure on this thread
 *    (the reference ops return false + LogError; never throw).
 *  - All data pointers are DEVICE pointers unless the name says host.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  No op
 *    synchronises; the reference's "synchronous on return" behaviour is
 *    obtained by calling ifa_stream_sync() after the op.
 *  - dtype ids are the reference's ElementType enum values
 *    (src/tensor/tensor_common.h:15-42).
 *  - Tensors are row-major with ne0 (columns) contiguous, like DeviceTensor
 *    (src/tensor/device_tensor.h:85-153).  Quantized rows hold
 *    cols/capacity blocks in the reference's byte layout
 *    (src/common/quant_types.h:11-174).
 */
#ifndef INFERFLOW_AMD_H_
#define INFERFLOW_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    IFA_F32 = 0, IFA_F16 = 1,
    IFA_Q8_B32T1 = 7, IFA_Q8_B32T2 = 8, IFA_Q6_B64T1 = 9, IFA_Q5_B64T1 = 10, IFA_Q5_B32T1 = 11,
    IFA_Q4_B16 = 12, IFA_Q4_B32T1A = 13, IFA_Q4_B32T1B = 14, IFA_Q4_B64T1 = 17, IFA_Q3H_B64T1 = 18,
    IFA_Q3_B32T1A = 19, IFA_Q3_B32T1B = 20, IFA_Q2_B32T1A = 21, IFA_Q2_B32T1B = 22
} ifa_dtype;

enum {
    IFA_OK = 0,
    IFA_ERR_ARG = -1,      /* bad shape / null pointer / misaligned size */
    IFA_ERR_DTYPE = -2,    /* dtype not supported by this op */
    IFA_ERR_HIP = -3,      /* HIP runtime error */
    IFA_ERR_STATE = -4,    /* object not initialised / wrong phase */
    IFA_ERR_NOMEM = -5
};

typedef void *ifa_stream;

/* ---- library ------------------------------------------------------------ */
const char *ifa_version(void);
const char *ifa_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int ifa_device_count(void);

/* ---- CudaUtil counterparts (src/common/cuda_util.h:40-61) --------------- */
int ifa_set_device(int device);
int ifa_malloc(void **dptr, size_t bytes);
int ifa_free(void *dptr);
int ifa_memcpy_h2d(void *dst, const void *src_host, size_t bytes, ifa_stream stream);
int ifa_memcpy_d2h(void *dst_host, const void *src, size_t bytes, ifa_stream stream);
int ifa_memcpy_d2d(void *dst, const void *src, size_t bytes, ifa_stream stream);
int ifa_memset(void *dst, int value, size_t bytes, ifa_stream stream);
int ifa_stream_create(ifa_stream *out);
int ifa_stream_destroy(ifa_stream s);
int ifa_stream_sync(ifa_stream s);

/* ---- type registry (src/tensor/tensor_common.cc:6-234) ------------------ */
int ifa_block_capacity(int dtype);               /* 0 if unknown */
int ifa_block_bytes(int dtype);
size_t ifa_row_bytes(int dtype, size_t cols);    /* TensorCommon::ByteCount per row */
/* "q4" -> IFA_Q4_B32T1A etc.; returns -1 if unknown (InitElementTypeMap :171-205) */
int ifa_dtype_from_name(const char *name);

/* ---- TensorOpr::Quantize / Dequantize (src/tensor/tensor_opr.cu:1623, :2229) */
/* src F16 [rows][cols] -> packed reference-layout blocks.  Q8_B32T2 uses the
 * device alg-2 quantizer (src/kernels/tensor_quant.h:44-82) like the reference. */
int ifa_quantize(int dtype, const void *src_f16, size_t rows, size_t cols, void *dst, ifa_stream stream);
int ifa_quantize_f32(int dtype, const void *src_f32, size_t rows, size_t cols, void *dst, ifa_stream stream);
int ifa_dequantize(int dtype, const void *src, size_t rows, size_t cols, void *dst_f16, ifa_stream stream);
/* activation / KV-row quantizer: F16 [rows][cols] -> Q8_B32T2, cols may be ragged */
int ifa_quantize_act_q8(const void *src_f16, size_t rows, size_t cols, void *dst, ifa_stream stream);

/* ---- TensorMul::Gemv_AX (src/tensor/tensor_mul.h:27, tensor_mul.cu:766-846) */
/* y[rows] (F16) = W[rows][cols] . x (+bias).  x_dtype is IFA_Q8_B32T2 (the
 * int8 x intN path, gemv.h:1499-1709; W must be one of the 7 eligible types)
 * or IFA_F16 (gemv.h:469-1497; any W type incl. IFA_F16).  bias may be NULL. */
int ifa_gemv(int w_dtype, const void *W, size_t rows, size_t cols,
             int x_dtype, const void *x, const void *bias_f16, void *y_f16, ifa_stream stream);

/* ---- prefill / batched linear layer (MatrixMultiplication's T>1 branch,
 * src/transformer/inference_worker.cc:2374-2415: TensorOpr::Dequantize + CublasEngine::GemmEx
 * F16xF16->F16 with fp32 accumulate + Transpose).  Y[tokens][rows] (F16) = X[tokens][cols] (F16)
 * . W[rows][cols]^T (+bias); W in any block format (reference layout) or F16.  No F16 copy of W exists: up to 128 tokens
 * every lane dequantises the blocks it needs into its MFMA operand registers (split-K kernels, weight-stream bound);
 * above 128 tokens (formats with blocks of <= 32 values) a workgroup dequantises its weight tile once per K step into
 * LDS and 256 x 256 / 128 x 256 / 128 x 128 output tiles are multiplied from there (v_mfma_f32_32x32x16_f16).
 * Every T runs these in-tree kernels: the library neither links nor loads a vendor GEMM. */
int ifa_gemm(int w_dtype, const void *W, size_t rows, size_t cols, const void *x_f16, size_t tokens,
             const void *bias_f16, void *y_f16, ifa_stream stream);
/* the large-tile kernel for tokens > 128 (default 1; 0: the smaller-tile kernels serve every T).  The tile kernels add the same
 * products in DIFFERENT orders (and the split-K form of the 128 x 128 tiles adds its two halves of K as first + second): results
 * agree within the F16 rounding of one product row, they are not bit-identical.  < 0 only queries; returns the previous setting */
int ifa_gemm_big_tiles(int on);

/* ---- launches that wait for sibling workgroups inside the launch (the fused QKV + attention step, the split-K halves of the
 * large-tile GEMM, the K parts of the 9..32-row GEMM).  They are chosen only when the whole waiting grid can be resident at once:
 * occupancy of the kernel x the CUs this process may use (ROC_GLOBAL_CU_MASK / HSA_CU_MASK are read; IFA_VISIBLE_CUS overrides).
 * Every wait is bounded (0.2 s); one that gives up leaves a code, the synchronising call (ifa_stream_sync, ifa_model_forward /
 * _decode / _decode_batch) returns IFA_ERR_STATE, and the waiting launches stay off for the rest of the process -- the HIP context
 * survives, the non-waiting kernels serve from there on.  IFA_NO_INLAUNCH_WAITS=1 (environment) starts the process that way;
 * per model: ifa_model_set_option "rows_kparts" / "gemm_splitk" / "fuse_attn" = 0.
 * host-only helpers (no device needed): the residency rule and the CU-mask reader behind that choice. */
int ifa_wait_grid_decision(int blocks_per_cu, int visible_cus, long long grid);      /* 1: the grid fits */
int ifa_visible_cus_from_mask(const char *mask_text, int device, int device_cus);    /* CUs the mask leaves for `device` */
int ifa_inlaunch_waits_enabled(void);
/* frees the scratch the prefill kernels keep for this stream on the current device (call before destroying a stream that ran
 * long-prompt attention; ifa_model_destroy / ifa_model_set_stream do it for the worker's) */
int ifa_gemm_release_stream(ifa_stream stream);

/* Re-tile reference-layout rows into the row-local plane layout the fused
 * decode kernels stream (DESIGN.md "HBM layout"): same bytes per row, row stride
 * padded to a multiple of 16 (ifa_tiled_row_bytes; 0 for types without a tiled
 * layout).  Supported for the AX8-eligible types; src and dst must not alias;
 * dst holds rows * ifa_tiled_row_bytes(dtype, cols) bytes. */
size_t ifa_tiled_row_bytes(int dtype, size_t cols);
int ifa_repack_weights(int dtype, const void *src, size_t rows, size_t cols, void *dst, ifa_stream stream);
/* same GEMV as ifa_gemv(x_dtype = Q8) reading the re-tiled layout */
int ifa_gemv_tiled(int w_dtype, const void *Wt, size_t rows, size_t cols,
                   const void *x_q8, const void *bias_f16, void *y_f16, ifa_stream stream);

/* ---- TensorOpr::LayerNormalization (tensor_opr.cu:458-602) --------------- */
/* kind 0 = RMS (x*rsqrt(mean(x^2)+eps)*(multi_base+w) + b), 1 = STD.  w,b may be NULL. */
int ifa_layernorm(int kind, const void *x_f16, size_t rows, size_t cols, const void *w_f16,
                  const void *b_f16, float multi_base, float eps, void *y_f16, ifa_stream stream);

/* ---- TensorOpr::PositionEmbedding (tensor_opr.cu:693-806) --------------- */
/* x F16 [tokens][heads][head_dim] in place; order 1 = adjacent pairs
 * (PosEmbedding_Rope_Std_Kernel), 2 = (c, c+rope_cols/2) (Rope_Order2). */
int ifa_rope(void *x_f16, int head_dim, int heads, int tokens, int pos0, float theta,
             int order, float partial_rotary_factor, ifa_stream stream);
/* scores F16 [heads][q_tokens][ctx] += col*m_head (PosEmbedding_Alibi_Std_Kernel) */
int ifa_alibi(void *scores_f16, int ctx, int q_tokens, int heads, int base_head, int total_heads,
              ifa_stream stream);

/* ---- TensorOpr::SoftMax (tensor_opr.cu:1189-1225) ------------------------ */
/* s F16 [cz][cy][cx] in place; element xi of row r is masked (-inf) iff
 * prefix_len >= 0 && xi > prefix_len + r; values are multiplied by scale first. */
int ifa_softmax(void *s_f16, int cx, int cy, int cz, int prefix_len, float scale, ifa_stream stream);

/* ---- TensorOpr::Activation / Mul / Add / Scale --------------------------- */
/* kind 0 silu, 1 gelu(tanh), 2 relu; is_glu: input rows are [2*cols], out = act(a)*b */
int ifa_activation(int kind, int is_glu, const void *x_f16, size_t rows, size_t cols, void *y_f16,
                   ifa_stream stream);
int ifa_mul(const void *a_f16, const void *b_f16, size_t n, void *c_f16, ifa_stream stream);
/* c = a + b, b broadcast with period b_period elements (0 = same size) */
int ifa_add(const void *a_f16, const void *b_f16, size_t n, size_t b_period, void *c_f16, ifa_stream stream);
int ifa_scale(const void *a_f16, float s, size_t n, void *c_f16, ifa_stream stream);
/* TensorOpr::AddByRowIndex (tensor_opr.cu:1519-1548, kernel binary_tensor_opr.h:80-125), the MoE scatter-add:
 * B[row_idx[r]][:] = hfma(A[r][:], weights[r], B[row_idx[r]][:]) in half precision (weights may be NULL = 1). */
int ifa_add_by_row_index(void *b_f16, const void *a_f16, size_t rows, size_t cols, const int *row_idx_dev,
                         const void *weights_f16_dev, ifa_stream stream);

/* ---- attention over a KV cache (inference_worker.cc:983-1405, :1639-1724) */
/* q F16 [q_tokens][heads][head_dim]; caches [n_ctx rows][kv_heads*head_dim] in
 * IFA_F16 or IFA_Q8_B32T2 (LayerKVCache, kv_cache.cc:104-249); causal mask with
 * prefix_len; GQA by indexing (no RepeatKV copy); out F16 [q_tokens][heads*head_dim].
 * alibi: 0/1; alibi_base_head/total_heads as in ifa_alibi. */
int ifa_attention(const void *q_f16, const void *kcache, const void *vcache, int kv_dtype,
                  int n_ctx, int q_tokens, int prefix_len, int heads, int kv_heads, int head_dim,
                  float kq_scale, int alibi, int alibi_base_head, int alibi_total_heads,
                  void *out_f16, ifa_stream stream);
/* ---- parity instruments: single-row ops in the SUMMATION ORDER of the reference's CUDA kernels (csrc/ifa_exact.hip) -- the 32-lane walk +
 * xor butterfly of Gemv_AX8_* (src/kernels/gemv.h:1499-1709; F16 activations: the serial fp32 order of the oracle's restatement of :469-1497),
 * Tensor_RmsNorm_Kernel's 128 chunks (unary_tensor_opr.h:216-289), serial fp32 attention dots + the 32-lane softmax (gemm.h:83-178,
 * unary_tensor_opr.h:480-535), SiLU / ReLU (+ gate) with libm's expf.  Results equal the CPU oracle's bit for bit; not timed kernels.
 * Same argument meaning as ifa_layernorm / ifa_gemv / ifa_attention (one query row, no ALiBi) / ifa_activation_mul (gate may be NULL). */
int ifa_exact_rmsnorm(const void *x_f16, size_t rows, size_t cols, const void *w_f16, const void *b_f16, float multi_base, float eps,
                      void *y_f16, ifa_stream stream);
int ifa_exact_gemv(int w_dtype, const void *W, size_t rows, size_t cols, int x_dtype, const void *x, const void *bias_f16, void *y_f16,
                   ifa_stream stream);
int ifa_exact_attention(const void *q_f16, const void *kcache, const void *vcache, int kv_dtype, int n_ctx, int heads, int kv_heads,
                        int head_dim, float kq_scale, void *out_f16, ifa_stream stream);
int ifa_exact_activation_mul(int kind, const void *a_f16, const void *gate_f16, size_t n, void *y_f16, ifa_stream stream);
/* chunks of at least min_tokens queries (default 64; 0 = never, < 0 only queries) take the two-pass kernels: K / V blocks staged
 * once per query tile, scores recomputed in the second pass instead of a [queries x keys] tile; head_dim 64 / 128; same rounding
 * points as the staged 32-query kernel.  Default variant: 64 queries per workgroup, the key blocks split over wave pairs;
 * on contexts of at least min_keys keys (default: never) chunks of >= 128 queries take the 128-query variant instead.
 * Each returns its previous threshold. */
int ifa_attention_two_pass_min(int min_tokens);
int ifa_attention_two_pass_min_keys(int min_keys);
/* dynamic batching: n_rows query rows, each ONE new token of its own query.  rows_dev: device array of n_rows records
 * { const void *kcache, *vcache; int n_ctx, pad; } -- row t attends to all n_ctx keys of its own caches; max_ctx: the longest of
 * them (it sizes the LDS).  q F16 [n_rows][heads][head_dim], out F16 [n_rows][heads*head_dim]; the rest as ifa_attention. */
int ifa_attention_rows(const void *q_f16, const void *rows_dev, int kv_dtype, int n_rows, int max_ctx, int heads, int kv_heads,
                       int head_dim, float kq_scale, int alibi, int alibi_base_head, int alibi_total_heads, void *out_f16,
                       ifa_stream stream);
/* What a call of ifa_attention / ifa_attention_rows launches (csrc/ifa_attn_plan.h).  Host-only, no GPU needed, no state.
 * facts[10], in the order of AttnFacts: kv_dtype, n_ctx, q_tokens, prefix_len, heads, kv_heads, head_dim, two_pass_min and
 * two_pass_min_keys (the values the two setters above return), rows_mode (1: ifa_attention_rows with n_ctx = max_ctx, q_tokens =
 * n_rows).  out[10], in the order of AttnPlan: error (0 ok, 1 kv dtype, 2 heads / kv_heads, 3 head_dim, 4 n_ctx / q_tokens / prefix,
 * 5 too long), kind (0 scalar k_attention, 1 MFMA tiles with the score tile in LDS, 2 the same with a global workspace, 3 two-pass
 * with 64 queries per workgroup, 4 two-pass with 128), queries per workgroup, grid x, grid y, dynamic LDS bytes, sg_nkp (row stride
 * of the workspace tiles, halfs), xcd_remap, then the workspace bytes as two ints (low half first). */
int ifa_attention_plan(const int *facts, int n_facts, int *out, int n_out);

/* ---- greedy argmax over F16 logits (SampleTokens top-1) ------------------ */
/* MoE routing of `tokens` softmaxed router rows [tokens][experts] on the device -- the per-row part of
 * HostTensorOpr::BuildRowsForMoE (src/tensor/host_tensor_opr.cc:190-244): top_k by repeated first maximum, probabilities
 * below 1e-5 dropped, optional renormalisation over the kept ones.  sel_out [tokens][top_k]: expert ids in ascending
 * order (-1 = unused slot), weights_out [tokens][top_k] F16.  (The reference copies the probabilities to the host.) */
int ifa_moe_route_topk(const void *probs_f16, size_t tokens, int experts, int top_k, int norm_top_k_prob, int *sel_out_dev,
                       void *weights_out_f16_dev, ifa_stream stream);
/* The three list kernels of the device-routed MoE layer (csrc/ifa_moe.h) on device pointers.  Enqueue-only, capturable.
 * ifa_moe_build_lists: from sel / wsel [tokens][top_k] (ifa_moe_route_topk's output; slots with an id outside [0, experts) are
 *   skipped) the entries in the reference's order -- experts ascending, token order inside an expert: idx_out[pos] = token row,
 *   wdev_out[pos] = its F16 weight, epos_out[t * top_k + j] = pos of row t's slot j (-1: none; every slot is written).
 *   tiles_out / smalls_out: records {int expert, row0, nrows, 0}; singles_out: {int expert, pos}; counts_out[0..3] = entries, tiles,
 *   singles, smalls.  An expert with 1 row is a single, with 2..small_max rows a small, otherwise ceil(rows / tile_rows) tiles in row
 *   order.  Capacities: tokens * top_k entries, entries / tile_rows + experts tiles, experts singles, min(experts, entries / 2) smalls.
 *   experts 1..64, top_k 1..8, tile_rows 64 or 128, small_max 0..8.
 * ifa_moe_gather: dst[pos][:] = src[idx[pos]][:] for pos < counts[0] (<= max_entries, the grid); dim % 8 == 0.
 * ifa_moe_combine: out[t][d] = residual[t][d] + sum_j y[epos[t][j]][d] * wsel[t][j] -- a half fma chain from 0 over the slots in
 *   order (AddByRowIdx), slots with epos -1 skipped, then the residual (nullable) as one half addition. */
int ifa_moe_build_lists(const int *sel_dev, const void *wsel_f16_dev, size_t tokens, int top_k, int experts, int tile_rows, int small_max,
                        int *idx_out_dev, void *wdev_out_f16_dev, int *epos_out_dev, void *tiles_out_dev, void *singles_out_dev,
                        void *smalls_out_dev, int *counts_out_dev, ifa_stream stream);
int ifa_moe_gather(const void *src_f16, const int *idx_dev, const int *counts_dev, size_t max_entries, size_t dim, void *dst_f16, ifa_stream stream);
int ifa_moe_combine(const void *y_f16, const int *epos_dev, const void *wsel_f16_dev, size_t tokens, int top_k, size_t dim, const void *residual_f16,
                    void *out_f16, ifa_stream stream);
/* LayerKVCache::SetKRows / SetVRows (src/transformer/kv_cache.cc:159-249): `tokens` F16 rows [kv_dim] into rows
 * [first_row, first_row + tokens) of a K or V cache of dtype F16 (copy) or Q8_B32T2 (the Alg2 quantiser) */
int ifa_kv_store(int kv_dtype, const void *rows_f16, size_t tokens, size_t kv_dim, void *cache, size_t first_row, ifa_stream stream);
int ifa_argmax(const void *logits_f16, size_t n, int *out_index_dev, ifa_stream stream);
/* the same over the ALLOWED ids: excluded_dev = {count (<= 3), id, id, id} in device memory (nullable) -- the ids
 * SamplingStrategy::GetSortedTopK never offers to its queue: the vocabulary's unk id and Invalid-type tokens
 * (src/transformer/sampling_strategy.cc:281-297) */
int ifa_argmax_masked(const void *logits_f16, size_t n, const int *excluded_dev, int *out_index_dev, ifa_stream stream);
#define IFA_POOL_MAX 256
/* SamplingStrategy::GetSortedTopK (src/transformer/sampling_strategy.cc:281-297) for `rows` logits rows [rows][n] F16:
 * per row the k best (value, id) pairs, best first; equal values: lower id first (+0.0 and -0.0 are equal); NaN never
 * enters; ids whose bit is set in excluded_bits_dev (nullable, ceil(n/32) words, bit id % 32 of word id / 32) are never
 * offered.  ids_out [rows][k] int32, vals_out [rows][k] F16 bits (the bits the row holds at that id), count_out [rows] =
 * min(k, admissible entries); slots past the count are unspecified.  1 <= k <= IFA_POOL_MAX.  Enqueue-only, capturable. */
int ifa_topk_pool(const void *logits_f16, size_t rows, size_t n, int k, const unsigned *excluded_bits_dev,
                  int *ids_out_dev, void *vals_out_f16_dev, int *count_out_dev, ifa_stream stream);
/* The softmax normaliser of `rows` F16 logits rows over the FULL vocabulary (no exclusion mask: the perplexity tool's softmax):
 * lse = max + log(sum exp(x - max)), x widened from F16, fp32 arithmetic; log p(id) = float(row[id]) - lse.  Row r is
 * logits + (row_idx_dev ? row_idx_dev[r] : r) * row_stride halfs (row_stride >= n).  targets_dev (nullable) holds one id per row;
 * target_logit_out_dev[r] (nullable) = the row's value at that id widened exactly, NaN for a target below 0.  -inf entries
 * contribute 0; lse is NaN exactly when the float64 definition is: a NaN or +inf in the row, or a row of -inf only.
 * Wave64, 16-byte loads, 2048 independent partial sums per workgroup and fixed reduction trees: no float atomics, run-to-run
 * identical.  With `rows` below 64 a row is split over up to 64 workgroups whose (max, sum) pairs a second small launch combines in
 * a fixed order; that needs workspace_dev of ifa_logsumexp_workspace(rows, n) bytes (0 bytes: no split).  A null workspace_dev
 * takes one workgroup per row whatever the row count.  Enqueue-only, capturable. */
size_t ifa_logsumexp_workspace(size_t rows, size_t n);
int ifa_logsumexp_rows(const void *logits_f16, size_t row_stride, const int *row_idx_dev, size_t rows, size_t n,
                       const int *targets_dev, float *lse_out_dev, float *target_logit_out_dev, void *workspace_dev, ifa_stream stream);

/* ---- the draw of the sampled strategies on a candidate pool (csrc/ifa_sample_rule.h, csrc/ifa_sample_pool.hip): everything
 * ChooseTokensFromPool does behind ifa_topk_pool for strategy_id 1 sample.std, 2 greedy, 3 top_k, 4 sample.top_p, 7 min_p.  Per row:
 * count (0..k) entries ids[] / F16 vals[] in the pool's order (value descending, lower id among equals), the parameters below and
 * the 48-bit state of the query's generator (java.util.Random's LCG; a generator seeded with s starts at (s ^ 0x5DEECE66D) & (2^48 - 1)).
 *   greedy: ids[0]; the generator is not touched.
 *   sort:   libstdc++'s std::sort under a.w > b.w restated (introsort, median of 3, runs of 16, heapsort below depth 2 floor(log2 n),
 *           final insertion sort): NOT stable, its order of equal F16 values decides ids.
 *   softmax: t = max(temperature, 0.001); e = (float)exp((double)((w - max) / t)); sequential float sum, floor 1e-5; p = e / sum.
 *   cut:    1 / 4: running float sum until >= top_p or min(count, max_k) entries; 3: the same with top_p = 1; 7: entries while
 *           p >= min_p * p[0] (the first always).
 *   draw:   interval starts in double (a NaN probability counts 0), r = NextDouble() * total, the reference's interval search.
 * The device's exp is ocml's double exp (1 ulp), the host's is libm's; rounded to float the two differ only where the double lies
 * within an ulp of a float rounding boundary.  Everything else is integer or correctly rounded IEEE arithmetic. */
typedef struct {
    int strategy_id;
    float temperature, top_p;
    int max_k;
    float min_p;
    int pool_size;      /* ifa_model_decode_sampled only: the pool length k of the step (1 for greedy); the two calls below ignore it */
} ifa_sample_params;
/* One wave per row, enqueue-only, capturable.  counts_dev [rows], ids_dev / vals_f16_dev [rows][k_stride] as ifa_topk_pool writes
 * them with k = k_stride (1..IFA_POOL_MAX); params_dev [rows]; rng_state_dev [rows] advances in place (by two steps per drawn
 * row); tokens_out_dev / index_out_dev [rows]: the drawn id and its index in the sorted pool; weights_out_dev (nullable)
 * [rows][k_stride]: the probabilities of the sorted pool (count per row; untouched for a greedy row).  A row that cannot be drawn --
 * count 0, an unknown strategy, a NaN value -- writes token / index -1, leaves its generator alone and stores row + 1 into
 * *err_dev if that word is 0 (clear it before the launch); the other rows are not affected. */
int ifa_sample_pool_rows(const int *counts_dev, const int *ids_dev, const void *vals_f16_dev, size_t rows, int k_stride,
                         const ifa_sample_params *params_dev, unsigned long long *rng_state_dev, int *tokens_out_dev, int *index_out_dev,
                         float *weights_out_dev, int *err_dev, ifa_stream stream);
/* host-only (no device needed): the same code compiled for the CPU, one row.  index_out / cut_len_out / weights_out [count] /
 * order_ids_out [count] (the ids in sorted order) are nullable.  IFA_ERR_STATE: count == 0 (no token); IFA_ERR_ARG: count outside
 * 0..IFA_POOL_MAX, an unknown strategy, a NaN value. */
int ifa_sample_pool_host(const int *ids, const unsigned short *vals_f16, int count, const ifa_sample_params *p,
                         unsigned long long *rng_state_inout, int *token_out, int *index_out, int *cut_len_out, float *weights_out,
                         int *order_ids_out);
/* The verify step of lookup decoding for seeded sampled queries: `rows` (1..8) pools of ONE query's draft step drawn as a chain.
 * draft_dev [rows - 1]: draft_dev[i] is the guess for the token row i emits (row i + 1 was computed behind it); ONE
 * ifa_sample_params and ONE generator state in device memory.  The specification:
 *   st = *rng; e = 0
 *   for i in 0 .. rows-1:
 *       draw row i by the rule of ifa_sample_pool_host with state st -> (tok, st')         (greedy: ids[i][0], st' = st)
 *       if the row cannot be drawn (empty pool, NaN, unknown strategy): if *err == 0: *err = i + 1; break
 *       tokens[e++] = tok; st = st'
 *       if i == rows-1 or tok != draft[i]: break
 *   *rng = st; *n_out = e; tokens[e..rows) = -1           (index_out_dev, nullable, likewise: the index in the sorted pool)
 * A row behind the first mismatch is never looked at: it can neither raise an error nor move the generator.  Since every sampled
 * draw advances the generator by exactly two steps, the tokens are exactly those of a row-by-row loop over the same pools.  One
 * workgroup of `rows` waves (wave i draws row i from the state 2 i steps on), one barrier, one lane scans; enqueue-only, capturable. */
int ifa_sample_verify_rows(const int *counts_dev, const int *ids_dev, const void *vals_f16_dev, size_t rows, int k_stride,
                           const ifa_sample_params *params_dev, const int *draft_dev, unsigned long long *rng_state_dev, int *tokens_out_dev,
                           int *index_out_dev, int *n_out_dev, int *err_dev, ifa_stream stream);
/* host-only (no device needed): the same chain on the CPU, built on ifa_sample_pool_host; the arrays are laid out as above.
 * *err_inout is left alone unless it is 0 and a reached row cannot be drawn.  IFA_ERR_ARG: rows / k_stride out of range, null pointers. */
int ifa_sample_verify_host(const int *counts, const int *ids, const unsigned short *vals_f16, int rows, int k_stride, const ifa_sample_params *p,
                           const int *draft, unsigned long long *rng_state_inout, int *tokens_out, int *index_out, int *n_out, int *err_inout);

/* ---- logit processors (csrc/ifa_logit_adjust.hip): repetition / frequency / presence penalties and logit_bias on F16 logits rows.
 * State per slot (one slot per query), dense over the n ids of the vocabulary, all in device memory owned by the caller:
 *   state_dev [slots][n] u32: bit 31 = the id occurs in the prompt, bits 0..30 = how many times it has been generated;
 *   bias_dev [slots][n] f32 (0: none, -inf bans the id); params_dev [slots][3] f32 = {rep, freq, pres}.
 * ifa_logit_adjust_rows: out row r (compact, stride n) from input row (row_idx_dev ? row_idx_dev[r] : r) of logits_f16
 * [.][row_stride] with the state of slot q = state_slot_dev[r].  Per id, fp32, every operation rounded on its own, in this order:
 *   x = float(in[id]); w = state[q][id]; c = w & 0x7fffffff;
 *   if (w != 0 && rep != 1) x = x > 0 ? x / rep : x * rep;          (the HF repetition rule: prompt + generated ids)
 *   x = x - (freq * float(c) + (c > 0 ? pres : 0));                  (the OpenAI rule: generated ids only)
 *   x = x + bias[q][id];
 *   bias[q][id] == -inf: -inf; else clamp to +-65504, round to F16 (RNE); a NaN is written as 0x7E00.
 * (Taken literally: an infinite input leaves as +-65504; -0.0 under neutral parameters leaves as +0.0.)  Pure, out of place,
 * enqueue-only, capturable; grid (ceil(n / 2048), rows), 16-byte accesses for a row whose four bases are 16-byte aligned, else id by id; no
 * atomics, run-to-run identical.  Slots in state_slot_dev must lie inside the three arrays. */
int ifa_logit_adjust_rows(const void *logits_f16, size_t row_stride, const int *row_idx_dev, const int *state_slot_dev, size_t rows, size_t n,
                          const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out_f16_dev, ifa_stream stream);
/* The rows of ONE slot's draft step (lookup decoding): `rows` (1..8) logits rows [rows][row_stride], row r computed behind the draft
 * tokens draft_dev[0..r) (draft_dev [rows - 1]); the slot is state_slot_dev[0].  Out row r (compact, stride n) is exactly what
 * ifa_logit_adjust_rows writes for input row r after ifa_logit_state_add of draft[0..r) to that slot: per id
 *   w' = w + #{j < r : draft[j] == id}       (bit 31 is kept, the count is w' & 0x7fffffff, the repetition rule fires on w' != 0)
 * and then the arithmetic above with w' in place of w -- the same inline function, same order, every operation rounded on its own.
 * Writes no state.  Same grid and access widths as ifa_logit_adjust_rows; enqueue-only, capturable. */
int ifa_logit_adjust_draft_rows(const void *logits_f16, size_t row_stride, const int *state_slot_dev, size_t rows, size_t n, const int *draft_dev,
                                const unsigned *state_dev, const float *bias_dev, const float *params_dev, void *out_f16_dev, ifa_stream stream);
/* clears the state and bias rows of `slot`, sets bit 31 for every prompt id (duplicates welcome), scatters the n_bias
 * (id, value) pairs into the bias row and writes {rep, freq, pres}; ids outside 0..n-1 are skipped.  Two memsets + one launch. */
int ifa_logit_state_reset(int slot, const int *prompt_tokens_dev, size_t n_prompt, float rep, float freq, float pres, const int *bias_ids_dev,
                          const float *bias_vals_dev, size_t n_bias, size_t n, unsigned *state_dev, float *bias_dev, float *params_dev, ifa_stream stream);
/* state[slots_dev[i]][tokens_dev[i]] += 1 for the n_pairs pairs in one launch (integer atomics: repeated pairs add up, the
 * result does not depend on the order); pairs outside [0, n_slots) x [0, n) are skipped */
int ifa_logit_state_add(const int *slots_dev, const int *tokens_dev, size_t n_pairs, size_t n, size_t n_slots, unsigned *state_dev, ifa_stream stream);

/* ---- the feed of a device-fed batched decode step (csrc/ifa_batch_feed.h, csrc/ifa_batch_feed.hip): what stands between two
 * batched steps of the same n rows when no host is in the loop.  Per row r of step s = *step:
 *   not live:   ring[s][r] = -1; pair_slot[r] = -1; nothing else of the row changes.
 *   live:       t = the row's token by its kind -- ARGMAX: argmax[r] (what the step's masked greedy pick wrote); POOL_BEST:
 *               pool_ids[j][0], entry 0 of the row's candidate pool (-1 for pool_counts[j] <= 0); DRAWN: drawn[j] (what
 *               ifa_sample_pool_rows wrote).  j = sel: a step pools and draws only the rows that need it, j is the row's place
 *               among them (as rows_sel of ifa_model_decode_batch_pool); a j outside 0 .. n-1 has no pool: t = -1.
 *     t < 0:    the row cannot go on (an empty pool, a NaN, a missing array, an unknown kind): live = 0, ring[s][r] = -1,
 *               pair_slot[r] = -1, and *err = 1 + s * n + r if that word is 0.  Of several such rows the first step's lowest row
 *               owns the word; later ones never overwrite it.
 *     else:     ring[s][r] = t; emitted += 1; rng_final = rng[j] for a j inside 0 .. n-1 (the generator as it stands behind this row's draw);
 *               pair_slot[r] = state_slot, pair_tok[r] = t (the pair ifa_logit_state_add counts; it skips a slot of -1);
 *               t among stop_ids[0 .. n_stop): live = 0 -- the row is frozen: it stays in the step, so that n and with it every
 *               other row's arithmetic does not change, and reprocesses the same token at the same position;
 *               otherwise tok[r] = t, pos[r] += 1 and attn_rows[l][r].n_ctx += 1 for every layer l.
 *   *step = s + 1.  A step outside 0 .. ring_steps-1 changes nothing and stores -1 into *err if that word is 0.
 * attn_rows is the batched step's attention table: [layers][n] entries of IFA_BATCH_ATTN_ROW_BYTES bytes (K cache pointer, V cache
 * pointer, int32 n_ctx at byte 16, int32 pad).  A frozen row's later draws move rng[j] but never rng_final, and nothing is
 * counted for it. */
#define IFA_BATCH_STOP_MAX 8
#define IFA_BATCH_ROWS_MAX 32
#define IFA_BATCH_STEPS_MAX 256
#define IFA_BATCH_LAYERS_MAX 1024
#define IFA_BATCH_ATTN_ROW_BYTES 24
enum { IFA_BATCH_KIND_ARGMAX = 0, IFA_BATCH_KIND_POOL_BEST = 1, IFA_BATCH_KIND_DRAWN = 2 };
typedef struct {
    int live, emitted, kind, n_stop;
    int stop_ids[IFA_BATCH_STOP_MAX];
    int state_slot, sel;
    unsigned long long rng_final;
} ifa_batch_feed_row;      /* 64 bytes */
typedef struct {
    int struct_size;                        /* sizeof(ifa_batch_feed_args) */
    int n, layers, ring_steps, k_stride, reserved;
    ifa_batch_feed_row *rows;               /* [n], in/out */
    int *step;                              /* [1], in/out */
    const int *argmax;                      /* [n], nullable */
    const int *pool_counts, *pool_ids;      /* [n], [n][k_stride]; nullable, both or neither */
    const int *drawn;                       /* [n], nullable */
    const unsigned long long *rng;          /* [n], nullable: rng_final is then left alone */
    int *tok, *pos;                         /* [n], in/out: the step's token and position tables */
    void *attn_rows;                        /* [layers][n], in/out (nullable for layers == 0) */
    int *ring;                              /* [ring_steps][n], out */
    int *pair_slot, *pair_tok;              /* [n], out */
    int *err;                               /* [1], in/out */
} ifa_batch_feed_args;
/* every array in device memory; one launch of one workgroup (the row's thread applies the row's rule, the attention entries are
 * spread over up to 1024 threads), vector stores only, no atomics; enqueue-only, capturable: what a step depends on -- the step
 * number included -- is read from device memory, never from the launch's arguments. */
int ifa_batch_feed_rows(const ifa_batch_feed_args *args_of_device_arrays, ifa_stream stream);
/* host-only (no device needed): the same code compiled for the CPU on host arrays */
int ifa_batch_feed_host(const ifa_batch_feed_args *args_of_host_arrays);
/* counts_dev[r] = min(counts_dev[r], pool_len_dev[r]) for `rows` rows: ifa_topk_pool builds every pool of a step with the step's
 * one k, a row draws from its own pool length; the pool is exact and ordered, so its first pool_len entries ARE the pool_len-pool.
 * Goes between ifa_topk_pool and ifa_sample_pool_rows.  Enqueue-only, capturable. */
int ifa_batch_clamp_counts(int *counts_dev, const int *pool_len_dev, size_t rows, ifa_stream stream);

/* ======================================================================== */
/* Per-device decode worker: counterpart of GpuInferenceWorker                */
/* (src/transformer/inference_worker.h:23-62, inference_worker.cc:234-340)    */
/* for the hyper-parameters of ModelSpec (src/transformer/model.h:72-151).    */
/* ======================================================================== */
typedef struct ifa_model ifa_model;

typedef struct {
    int dim, layers, heads, kv_heads, head_dim, ffn, vocab, max_ctx;
    int norm_kind;       /* 0 rms, 1 std                      (normalization_function) */
    int act_kind;        /* 0 silu, 1 gelu, 2 relu            (activation_function)    */
    int is_glu;          /* informational: w3 present                                   */
    int rope_order;      /* 0 none, 1 adjacent pairs, 2 half-split (qk_column_order)    */
    int use_alibi;       /* position_embedding == alibi                                 */
    int parallel_attn;   /* is_parallel_attn                                            */
    int share_input;     /* mlp_attn_share_input                                        */
    float rope_theta, partial_rotary, kq_scale, eps;
    int kv_dtype;        /* IFA_F16 or IFA_Q8_B32T2 (device_kv_cache_data_type)         */
    int full_quant_gemv; /* enable_full_quant_gemv (inference_engine.cc:57)             */
    int experts, moe_top_k, moe_norm_topk;
    int tp_rank, tp_size;/* tensor-parallel shard of this worker (heads/kv_heads/ffn are per-shard) */
    int device;          /* HIP device ordinal */
    /* RMS weight = base + w (attn_pre_norm_base / ffn_pre_norm_base / output_norm_base: Gemma) and TensorOpr::Scale of
     * the attention output, the FFN output and the last layer's output (attn_out_scale / ffn_out_scale / out_scale:
     * MiniCPM; inference_worker.cc:568-570, 842-843, 928-929).  Scales <= 0 mean 1. */
    float attn_norm_base, ffn_norm_base, out_norm_base, attn_out_scale, ffn_out_scale, out_scale;
    /* TensorOpr::LinearNorm on the decoder input (has_embedding_linear_norm / embedding_linear_scale: Gemma, MiniCPM;
     * inference_worker.cc:447-451, tensor_opr.cu:482-497): every embedding row is multiplied by this scale;
     * 0 = absent, < 0 = the reference's default sqrt(dim). */
    float embd_scale;
} ifa_model_config;

/* tensor ids for ifa_model_set_tensor (StdDeviceNetwork, src/transformer/model.h:168-276) */
enum {
    IFA_T_EMBD = 0, IFA_T_OUT_NORM = 1, IFA_T_OUT_NORM_B = 2, IFA_T_LM_HEAD = 3,
    IFA_T_ATTN_NORM = 10, IFA_T_ATTN_NORM_B = 11, IFA_T_WQ = 12, IFA_T_WK = 13, IFA_T_WV = 14, IFA_T_WO = 15,
    IFA_T_FFN_NORM = 16, IFA_T_FFN_NORM_B = 17, IFA_T_W1 = 18, IFA_T_W2 = 19, IFA_T_W3 = 20, IFA_T_MOE_GATE = 21,
    IFA_T_WQ_B = 22, IFA_T_WK_B = 23, IFA_T_WV_B = 24, IFA_T_WO_B = 25, IFA_T_W1_B = 26, IFA_T_W2_B = 27, IFA_T_W3_B = 28,
    /* self_attn.post_norm / feed_forward.post_norm (+ biases): StdDeviceNetwork::AttentionLayer::post_norm, FeedForwardLayer::post_norm
     * (src/transformer/model.h:168-276); applied by ProcessGpuLayer (inference_worker.cc:857-866, 954-965).  Models that carry them take
     * the op-by-op layer (the fused decode / prompt launches decline).  ModelSpec::is_attn_post_as_residual (model.h:113, default
     * true) is the model option "attn_post_as_residual". */
    IFA_T_ATTN_POST_NORM = 29, IFA_T_ATTN_POST_NORM_B = 30, IFA_T_FFN_POST_NORM = 31, IFA_T_FFN_POST_NORM_B = 32
};

int ifa_model_create(const ifa_model_config *cfg, ifa_model **out);
int ifa_model_destroy(ifa_model *m);
/* Copy a tensor that is already in its final dtype (reference block layout or F16)
 * from device memory into the worker; eligible weight matrices are also re-tiled. */
int ifa_model_set_tensor(ifa_model *m, int layer, int tensor_id, int expert, int dtype,
                         const void *dev_src, size_t rows, size_t cols);
/* F16 source quantised on the device to target_dtype first
 * (DeviceTensorBuilder::Build_Quant, src/tensor/device_tensor_builder.cu:383-420). */
int ifa_model_set_tensor_f16(ifa_model *m, int layer, int tensor_id, int expert, int target_dtype,
                             const void *dev_src_f16, size_t rows, size_t cols);
/* allocate KV caches (KVCache::Init, kv_cache.cc:278-319) and scratch */
int ifa_model_finalize(ifa_model *m);
int ifa_model_reset(ifa_model *m);
/* options: "fused" (1), "graph" (1), "rpw_qkv|rpw_wo|rpw_ffn|rpw_w2|rpw_lm" (0 = auto), "batch_fused" (1), "rows_mo" (1: the batched
 * step and short prompts stream MFMA-operand-order copies of the weights, built on first use), "attn_split_ctx" (-1 = by model: 512 keys, 640 with grouped queries, 320 without the fused launch; a decode call that reaches more keys than this runs the attention as scores / P.V / combine launches with a head's keys split over 8 or 16 workgroups; 0: never), "fuse_attn" (1: the attention as the
 * tail of the wq | wk | wv launch), "attn_unload" (1: in the 256-row bucket of that launch the heads' workgroups take no weight rows and request their cache rows at once; 2: in the 128-row bucket too, measured slower), "fuse_ffn" (0; 1 / 2: [Wo ->] W1 | W3 -> W2 as one chained launch, csrc/ifa_decode_chain.h: bit-identical,
 * measured slower than the separate launches on MI355X, kept as the measurement harness of that statement), "prefill_mid" (1),
 * "prefill_mid_max" (768), "prefill_res_mid" (2048: up to this many tokens wo / w2 keep the mid-size kernel above prefill_mid_max), "prefill_big_min" (47), "attn_post_as_residual" (1), "exact_order" (0; 1: every single-token step -- and every row
 * of a prompt, one by one -- runs in the summation order of the reference's CUDA kernels, csrc/ifa_exact.hip: a parity instrument whose
 * logits, ids and int8 codes equal the CPU oracle's bit for bit; fails for models outside that step instead of changing arithmetic),
 * "q3h_native" (0; 1: Q3H_B64T1 Wo / W1 / W3 / W2 streamed at 32 bytes per block, pair codes decoded in the kernel: bit-identical, measured slower),
 * "perf_stat" (0; 1: steps and prompts take the op-by-op layer with a HIP event pair around every phase, see ifa_model_perf_stat) */
/* Independent KV caches inside one worker, one per concurrent query -- the reference keeps a LayerKVCache set
 * per query processor (QueryStateTable, src/transformer/query_state_table.h:19-85; KVCache::Init, kv_cache.cc:278-319).
 * ifa_model_kv_slots grows the number of caches to n_slots (slot 0 exists after finalize); ifa_model_select_kv
 * makes one of them the cache that forward()/decode() read and write (each slot keeps its own captured graph). */
int ifa_model_kv_slots(ifa_model *m, int n_slots);
int ifa_model_select_kv(ifa_model *m, int slot);
/* Rows [0, n_rows) of the K and V cache of every layer from slot src_slot to slot dst_slot -- what a prompt prefix cache needs
 * when the slot that holds a prompt's leading rows belongs to a running query (the engine's `prefix_cache` key).  ONE launch on
 * the model's stream for all 2 * layers segments (csrc/ifa_kv_copy.hip), ordered with the steps around it, no host
 * synchronisation; either slot may be the selected one.  The copy is byte for byte: a step on the destination behind the copied
 * rows computes what it would on the source.  n_rows = 0 is IFA_OK without a launch.  IFA_ERR_ARG: src_slot == dst_slot, a slot
 * outside ifa_model_kv_slots, n_rows outside 0..max_ctx, a model that is not finalized; IFA_ERR_STATE: a stream under capture. */
int ifa_model_kv_copy(ifa_model *m, int src_slot, int dst_slot, int n_rows);
/* Context shift (csrc/ifa_kv_shift.hip; arithmetic in DESIGN.md "Context shift"): of the n_rows cache rows of query slot `slot`
 * the rows [keep, keep + discard) are dropped and the rows [keep + discard, n_rows) of every layer's K and V move to
 * [keep, n_rows - discard).  V rows move byte for byte; K rows, which are stored with RoPE applied, are rotated back by `discard`
 * positions on the way (table: (cos, -sin) of position `discard` from the rope function of the steps' own tables), Q8_B32T2 rows
 * through dequantise / rotate / the store quantiser; a model without RoPE moves K byte for byte too.  Rows [0, keep), every byte
 * from row n_rows - discard on and every other slot are not written.  All 2 * layers segments go through the slot table in one
 * launch when the moved rows do not outnumber the dropped ones, else in ascending pieces of `discard` rows; on the model's stream,
 * ordered with the steps around it, no host synchronisation; either the selected slot or another one.  IFA_ERR_ARG: keep < 0,
 * discard < 1, keep + discard > n_rows, n_rows > max_ctx, an unknown slot, a Q8 cache whose head_dim is no multiple of 32, a model
 * that is not finalized; IFA_ERR_STATE: a stream under capture, a partitioned worker (tp_size > 1 or a topology). */
int ifa_model_kv_shift(ifa_model *m, int slot, int keep, int discard, int n_rows);
/* The same on ONE layer's pair of buffers ([rows][kv_heads * head_dim] halfs, or Q8_B32T2 blocks) with the caller's table:
 * table_dev = head_dim / 2 pairs (c, s) of fp32 on the device; pair (i0, i1) of a K row becomes (x0 * c - x1 * s, x0 * s + x1 * c).
 * rope_order 1: pairs (2 i, 2 i + 1); 2: pairs (i, i + rope_cols / 2) for 2 i < rope_cols, the other columns move verbatim; 0: K
 * moves like V (no table).  kcache / vcache may be NULL to skip a side; they need not start an allocation (the access width follows their alignment too), an
 * odd address is IFA_ERR_ARG.  kv_dtype: IFA_F16 or IFA_Q8_B32T2. */
int ifa_kv_shift_rows(int kv_dtype, void *kcache, void *vcache, size_t kv_heads, size_t head_dim, int rope_order, int rope_cols,
                      const float *table_dev, size_t keep, size_t discard, size_t n_rows, ifa_stream stream);
int ifa_model_set_option(ifa_model *m, const char *name, int value);
/* up to 3 token ids the worker's greedy argmax (forward / decode / decode_batch) never selects: the unk id and
 * Invalid-type tokens GetSortedTopK skips (sampling_strategy.cc:281-297).  None by default at this level; the engine
 * facade sets the model's unk id. */
int ifa_model_set_excluded_tokens(ifa_model *m, const int *ids_host, int n);
/* Per-phase times in the key space of the reference's InferencePerfStat (GpuInferenceWorker::UpdatePerfStat, inference_worker.cc:2670-2697;
 * keys: (layer + 1) * 10000 + phase -- + 0 the whole layer for layers 0..5 (:318-322); for layer 0, the reference's layer_idx_for_study_:
 * + 10 attention pre-norm, + 30 q / k / v products, + 50 RoPE + cache rows, + 60 scores / softmax / V product, + 90 wo, + 300 the attention
 * part as a whole, + 710 FFN pre-norm, + 730 w1, + 750 w3, + 760 activation * gate, + 780 w2, + 700 the FFN as a whole, + 800 what follows it;
 * 1000009 the output stage (:673-675), 1 the embedding rows (inference_engine.cc:1168-1176)).  With option "perf_stat" = 1 every
 * ifa_model_forward / ifa_model_decode step ADDS the device milliseconds of its spans to the keys (the reference adds host-side launch times);
 * this call drains the stream, copies up to cap (key, ms) pairs in ascending key order, stores the number of keys there are in *n_out and
 * clears the map if clear != 0. */
int ifa_model_perf_stat(ifa_model *m, int *keys_out, float *ms_out, int cap, int *n_out, int clear);
/* 1 if the fused batch-1 decode kernels cover this model, else 0 (+ reason) */
int ifa_model_fused_supported(ifa_model *m, char *why, size_t why_len);
/* One Infer() step for one query: n_tokens new tokens at positions
 * [prefix_len, prefix_len+n_tokens); op-by-op; synchronous.  logits_out_dev (F16
 * [n_tokens][vocab], nullable) mirrors return_output_tensors; *next_token_host is
 * the greedy argmax of the last row. */
int ifa_model_forward(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len,
                      void *logits_out_dev, int *next_token_host);
/* Greedy batch-1 decode of n_steps tokens starting from first_token at start_pos
 * (its KV rows [0,start_pos) must already be cached).  Fused kernels, one graph
 * replay per token, token fed back on the device.  out_tokens_host[n_steps]
 * receives the generated ids; *elapsed_ms (nullable) the HIP-event time of the
 * n_steps replays on the worker's stream. */
int ifa_model_decode(ifa_model *m, int first_token, int start_pos, int n_steps,
                     int *out_tokens_host, float *elapsed_ms);
/* ifa_model_decode with the token of every step DRAWN on the device (csrc/ifa_engine_sampled.hip): same arguments and semantics,
 * same fused kernels, one graph replay per token, one synchronisation per call.  The captured step gathers its own input and
 * ends in lm_head -> [ifa_logit_adjust_rows with the state of state_slot] -> ifa_topk_pool with k = p->pool_size and the mask of
 * ifa_model_set_pool_excluded -> the rule of ifa_sample_pool_rows + the advance of the device state -> [ifa_logit_state_add of the
 * drawn token to state_slot].  state_slot = -1: no logit processors; else a slot ifa_model_logit_state_reset has prepared: every
 * drawn token is counted there exactly once, before the next step reads the slot (first_token is NOT counted by this call).
 * *rng_state_inout: the generator state the first draw starts from; on success the state behind the last draw (n_steps draws of
 * two steps each; untouched for greedy).  Parameters, generator state, slot and error word travel through device memory written
 * by the call, so one captured step serves every query with the same (KV slot, pool_size, processors or not); the greedy step's
 * graphs are separate and stay valid.  Tokens equal, step for step, ifa_model_decode_pool + ifa_sample_pool_host on the same
 * logits.  IFA_ERR_STATE: a step whose pool was empty (message names the step; the call's results are not valid), options
 * exact_order / perf_stat / fused = 0, a model the fused step does not cover, a partitioned worker, embeddings / lm_head missing;
 * IFA_ERR_ARG: an unknown strategy, pool_size outside 1..IFA_POOL_MAX, a slot without logit state, ifa_model_decode's own checks. */
int ifa_model_decode_sampled(ifa_model *m, int first_token, int start_pos, int n_steps, const ifa_sample_params *p,
                             unsigned long long *rng_state_inout, int state_slot, int *out_tokens_host, float *elapsed_ms);
/* Everything a decode call of n_steps from start_pos sets up before its first launch (the attention variant of the contexts it
 * reaches, the hand-off arenas, the captured step and its multi-step replay) WITHOUT running a step: a caller that times its
 * first call keeps graph capture / instantiation out of it.  The KV cache and the activations are not touched. */
int ifa_model_decode_prepare(ifa_model *m, int start_pos, int n_steps);
/* Dynamic batching: ONE new token for each of n queries in one step (QueryStateTable + Infer_Std over several queries,
 * src/transformer/inference_engine.cc:1054-1220).  Row r is token tokens[r] at position positions[r] of the query whose
 * KV cache is slot kv_slots[r] (ifa_model_kv_slots; slots must be distinct).  The linear layers run once over the n rows
 * (the weights are streamed once for all queries), attention per row on its own cache.  logits_out: optional [n][vocab] F16. */
int ifa_model_decode_batch(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                           int *next_tokens_host, void *logits_out_dev);
/* The draft step (lookup / speculative decoding, csrc/ifa_decode_draft_kv.hip): n rows (2..8) of ONE query as one batched step on
 * the SELECTED KV slot.  Row i is tokens_host[i] at position pos0 + i behind cache rows [0, pos0 + i): row 0 the query's last
 * committed token (not yet in the cache), rows 1 .. n - 1 draft tokens.  next_tokens_host[i] = the masked greedy argmax of row i
 * (exclusions and tie rule of ifa_model_decode_batch); logits_out_dev: optional [n][vocab] F16 (a call with it runs eagerly, one
 * without replays a graph captured per n).  One synchronisation per call.  Row i is bit for bit -- logits, id, the K / V row it
 * writes -- the row ifa_model_decode_batch computes for a query at position pos0 + i whose slot holds the same bytes in rows
 * [0, pos0 + i).  Afterwards cache rows pos0 .. pos0 + n - 1 hold the n rows' K / V; the caller decides how many count (the
 * leading i with next[i - 1] == tokens[i]) and later steps overwrite the others.  IFA_ERR_ARG: n outside 2..8, pos0 < 0,
 * pos0 + n > max_ctx; IFA_ERR_STATE: a partitioned worker (tp_size > 1 or a topology), options exact_order or perf_stat. */
int ifa_model_decode_draft(ifa_model *m, int n, const int *tokens_host, int pos0, int *next_tokens_host, void *logits_out_dev);
/* The draft step for a seeded SAMPLED query (csrc/ifa_engine_draft_sampled.hip): ifa_model_decode_draft's step on the same n rows --
 * the same captured graph, cache rows pos0 .. pos0 + n - 1 bit for bit what that call writes -- followed on the worker's stream by
 * [ifa_logit_adjust_draft_rows with the state of state_slot (-1: no processors), draft = tokens_host[1..n)] -> ifa_topk_pool over the n
 * rows with k = p->pool_size and the mask of ifa_model_set_pool_excluded -> ifa_sample_verify_rows with *rng_state_inout.  One
 * synchronisation per call; parameters, drafts and generator state travel through device memory written by the call.
 * out_tokens_host [n]: the *n_out (1..n) emitted tokens, -1 behind them: token i is the draw of row i, rows 1 .. *n_out - 1 were
 * reached because tokens_host[i] equalled the draw of row i - 1; the caller keeps cache rows pos0 .. pos0 + *n_out - 1.  The tokens,
 * *n_out and the generator state equal ifa_sample_verify_host on the pools of the step's (adjusted) logits rows.  The call never
 * writes the logit state -- the caller counts the emitted tokens -- and leaves the greedy, draft and sampled graphs valid.
 * IFA_ERR_ARG: n outside 2..8, pos0 < 0, pos0 + n > max_ctx, an unknown strategy, pool_size outside 1..IFA_POOL_MAX, a slot without
 * logit state; IFA_ERR_STATE: a partitioned worker, lm_head missing, options exact_order or perf_stat, a reached row with an
 * empty pool (the message names the row; the results are not valid). */
int ifa_model_decode_draft_sampled(ifa_model *m, int n, const int *tokens_host, int pos0, const ifa_sample_params *p,
                                   unsigned long long *rng_state_inout, int state_slot, int *out_tokens_host, int *n_out);
/* ---- steps that end in a candidate pool (sampled decoding without the logits row on the host): ifa_topk_pool runs on the
 * step's logits on the worker's stream, in front of the step's ONE synchronisation, and (count, ids, values) come back
 * in one copy through pinned staging.  Everything after the pool -- softmax, cuts, the draw -- stays with the caller.
 * Partitioned workers (tp_size > 1, or a step driven through ifa_model_tp_*) return IFA_ERR_STATE; options exact_order
 * and perf_stat keep their own step (ifa_model_decode's fallbacks) and end in the same pool, the batched form under
 * exact_order returns IFA_ERR_STATE. */
/* device-resident mask of ids the pool never offers (any count); n = 0 clears it */
int ifa_model_set_pool_excluded(ifa_model *m, const int *ids_host, int n);
/* ifa_model_decode(first_token, start_pos, 1 step) followed by the pool of that step's logits row; the greedy id in
 * *next_token_host as before.  Takes whatever route ifa_model_decode takes for this model (fused + graph where
 * supported, else its fallback).  pool_ids_host / pool_vals_host hold k entries, *pool_count_host of them are valid. */
int ifa_model_decode_pool(ifa_model *m, int token, int pos, int k, int *next_token_host,
                          int *pool_ids_host, unsigned short *pool_vals_host, int *pool_count_host);
/* the same behind a batched step: rows_sel_host[n_sel] = strictly ascending indices (into the step's n rows) whose pools
 * are wanted; pool_ids_host / pool_vals_host [n_sel][k], pool_counts_host [n_sel] */
int ifa_model_decode_batch_pool(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                                int *next_tokens_host, int k, const int *rows_sel_host, int n_sel,
                                int *pool_ids_host, unsigned short *pool_vals_host, int *pool_counts_host);
/* the same behind a prompt step: ifa_model_forward(tokens, n_tokens, prefix_len, logits_out_dev) + the pool of the LAST row.
 * logits_out_dev as in ifa_model_forward (nullable); it also selects that call's arithmetic -- with it the lm_head runs over all
 * rows (the rows GEMM), without it over the last row only -- so a caller that wants the pool of exactly the logits
 * ifa_model_forward(..., logits_out_dev) produces passes the same buffer. */
int ifa_model_forward_pool(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev, int k,
                           int *next_token_host, int *pool_ids_host, unsigned short *pool_vals_host, int *pool_count_host);
/* Option "pool_lse" = 1 (ifa_model_set_option; default 0): the three pool steps above also run ifa_logsumexp_rows over every pooled
 * row and its lse rides in the same staged block; after the step ifa_model_pool_lse copies out the n_sel (1 for the single-query
 * steps) values, log p(pool id) = float(pool value) - lse.  With the option off the steps enqueue exactly what they did before and
 * *n_out is 0.  Changing the option keeps the captured graphs. */
int ifa_model_pool_lse(ifa_model *m, float *lse_host, int cap, int *n_out);
/* ---- logit processors behind the pool steps (csrc/ifa_logit_adjust.hip; state per KV slot, allocated on first use).
 * ifa_model_logit_state_reset: the state of the query in kv_slot -- clears it, marks the n_prompt prompt ids, stores the penalties
 * and the n_bias (id, value) logit_bias pairs (host pointers).  IFA_ERR_ARG with a message: rep not finite or <= 0, freq / pres
 * not finite, n_bias > IFA_LOGIT_BIAS_MAX, a bias id outside the vocabulary or given twice, a bias value that is neither finite
 * nor -inf, a prompt id outside the vocabulary, a slot outside ifa_model_kv_slots.  Synchronises the worker's stream.
 * ifa_model_logit_state_add: one more generated occurrence for each of the n (kv slot, token) pairs (n <= 1024), enqueued on the
 * worker's stream through pinned staging -- no synchronisation (a ring of 8 staging blocks; only a 9th call without any
 * synchronisation of the stream in between would wait for the first).
 * ifa_model_pool_adjust: arms the NEXT pool step (ifa_model_decode_pool / _decode_batch_pool / _forward_pool): entry j is the
 * state slot of pooled row j (1 entry for the single-query steps), -1 for a row that stays raw.  Armed rows pass through
 * ifa_logit_adjust_rows into the worker's buffer "logits_adj" ([pooled rows][vocab], row j at j * vocab) and the pool and the
 * log-sum-exp read that; the exclusion mask still applies; the "logits" buffer stays raw.  The arm is consumed by that step
 * whether it succeeds or fails; a step whose n_sel differs from n_sel here fails with IFA_ERR_ARG.  With nothing armed a step
 * enqueues exactly what it did before.  All three: IFA_ERR_STATE on a partitioned worker (tp_size > 1). */
#define IFA_LOGIT_BIAS_MAX 1024
int ifa_model_logit_state_reset(ifa_model *m, int kv_slot, const int *prompt_host, int n_prompt, float rep, float freq, float pres,
                                const int *bias_ids_host, const float *bias_vals_host, int n_bias);
int ifa_model_logit_state_add(ifa_model *m, int n, const int *kv_slots_host, const int *tokens_host);
int ifa_model_pool_adjust(ifa_model *m, int n_sel, const int *state_slots_host);
/* ---- device-fed batched steps (csrc/ifa_engine_batch_steps.hip): n_steps (1..256) batched steps of the same n rows with ONE
 * synchronisation.  The call equals n_steps calls of ifa_model_decode_batch -- or, for a row that is not plainly greedy, of
 * ifa_model_decode_batch_pool behind ifa_model_pool_adjust -- for the same rows in the same order, each followed by the feed rule
 * of ifa_batch_feed_rows with ifa_sample_pool_rows as the draw and ifa_logit_state_add of the rule's (slot, token) pairs: tokens,
 * generator words, logit state and every K / V byte written are identical.  Row r (nullable rows: all greedy, no stop ids, no
 * processors): p.strategy_id 1 / 2 / 3 / 4 / 7 with its parameters; a row is pooled unless it is greedy with state_slot -1; the
 * step's one pool length is the largest p.pool_size among the pooled rows and row r draws from its first
 * min(count, p.pool_size) entries (ifa_batch_clamp_counts); rng_state is the row's 48-bit generator word, on return the word
 * behind the row's last own draw; state_slot >= 0 passes the row's logits through the processors of that slot and counts every
 * token the row emits there; a row that emits one of its n_stop (0..IFA_BATCH_STOP_MAX) stop_ids is frozen: it stays in the
 * later steps of the call, reprocesses its last token at its last position (rewriting the same cache row with the same bytes) and
 * emits nothing.  out_tokens_host [n_steps][n]: the emitted tokens, -1 where the row was frozen; emitted_host [n].
 * How: the tables of the first step are uploaded once; every step replays a captured graph of its own per n -- the step of
 * ifa_model_decode_batch without the table upload and the copy back -- and the processors, pool, clamp, draw, feed and count
 * launches follow it on the stream; the call's values travel through device memory written by the call.  The graphs of the other
 * entry points are neither re-captured nor changed.  elapsed_ms (nullable): device time of the steps from HIP events.
 * IFA_ERR_STATE, nothing touched: the step of n rows is not ONE fused, captured step (ifa_batch_route_plan: n = 1, a chunked n,
 * an op-by-op model, options exact_order / perf_stat / graph = 0, a partitioned worker; the message says which).  IFA_ERR_ARG:
 * n_steps outside 1..256, a position with pos + n_steps > max_ctx, a slot used twice or outside the worker's, a token outside
 * the vocabulary, an unknown strategy, pool_size outside 1..IFA_POOL_MAX, n_stop outside 0..8, a state slot without logit state,
 * a struct_size that is not this header's.  IFA_ERR_STATE after the steps: a row had no token to draw (an empty pool); the message
 * names step and row and the results are not valid. */
typedef struct {
    int struct_size;                 /* sizeof(ifa_batch_row) */
    ifa_sample_params p;
    int state_slot;                  /* -1: no logit processors */
    unsigned long long rng_state;    /* in/out */
    int n_stop;
    int stop_ids[IFA_BATCH_STOP_MAX];
    int reserved;
} ifa_batch_row;
int ifa_model_decode_batch_steps(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host,
                                 int n_steps, ifa_batch_row *rows, int *out_tokens_host, int *emitted_host, float *elapsed_ms);
/* the most rows ifa_model_decode_batch_steps takes on this worker with its options as they stand (32 or 16; every n from 2 up to it
 * is one fused, captured step); 0: the call is refused whatever n.  Plans only, builds nothing. */
int ifa_model_batch_steps_rows(ifa_model *m);
/* A scoring prompt: ifa_model_forward(tokens, n_tokens, prefix_len) with the lm_head over ALL rows into the worker's own logits
 * buffer -- bit for bit the rows ifa_model_forward(..., logits_out_dev) delivers, on the same route (one pass, the two passes of a
 * 34..48-token prompt, options exact_order and perf_stat) -- then ifa_logsumexp_rows over them: lse_host[i] and
 * target_logit_host[i] = float(row i at targets_host[i]) (NaN for a target below 0) come back as 2 * n_tokens floats through pinned
 * staging in front of the prompt's one synchronisation.  log p(targets[i] | tokens[0..i]) = target_logit[i] - lse[i].  No
 * [n_tokens][vocab] block is allocated by the caller or copied.  *next_token_host (nullable) as in ifa_model_forward.  Partitioned
 * workers (tp_size > 1, or a topology) return IFA_ERR_STATE. */
int ifa_model_forward_score(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, const int *targets_host,
                            float *lse_host, float *target_logit_host, int *next_token_host);
/* debugging taps: "logits", "logits_adj" (the rows the last armed pool step adjusted; null before the first), "logit_state" (the
 * logit processors' u32 state rows [slots][vocab]; null before the first reset), "hidden", "kcache", "vcache" (device pointers).
 * "x", "att", "a", "t1", "hidden": ONE row.  "rows_x", "rows_xn", "rows_hn", "rows_att", "rows_a", "rows_t1", "rows_q", "rows_k", "rows_v": all
 * the rows (scratch_tokens of them: as many as the largest step so far) of the row-major activation buffers a batched or prompt step uses;
 * "rows_bqkv": the batched step's [32][q | k | v] (null before the first step of <= 32 rows).  "rows_f": the FFN output rows.
 * The device-routed MoE layer's buffers (models with experts; cap = scratch_tokens x top_k entries): "moe_gate" [rows][experts] F16
 * probabilities; "moe_sel" / "moe_selw" [cap] int / F16; "moe_idx", "moe_wdev", "moe_epos" [cap]; "moe_counts" (16 ints, the first 4 used);
 * "moe_tiles" (cap / 64 + experts + 1 records of 4 ints), "moe_singles" (experts + 1 records of 2 ints), "moe_smalls" (experts + 1 records
 * of 4 ints); "moe_gin", "moe_gout" [cap][dim]; "moe_g1", "moe_g3" [cap][ffn].  For reading: the worker's next step overwrites them. */
int ifa_model_get_buffer(ifa_model *m, const char *name, int layer, void **dptr, size_t *bytes);
void *ifa_model_stream(ifa_model *m);
/* Test hooks over the worker's memory (every device / pinned block a model owns goes through two counted allocators,
 * csrc/ifa_buf_hip.h).  Process-global; the countdown is not meant for concurrent use.
 * ifa_debug_alloc_fail_at: the nth such allocation from now on reports out of memory, once, without calling HIP (its message
 *   contains "simulated"); 0 disarms.
 * ifa_debug_live_allocs: the blocks (and their bytes) handed out and not yet freed; either pointer may be null.  The process-level
 *   caches of the GEMM / attention / runtime units are not counted. */
int ifa_debug_alloc_fail_at(long long nth);
int ifa_debug_live_allocs(long long *count, long long *bytes);
/* run the worker on a caller-owned stream (e.g. the one the caller's RCCL collectives are ordered on) */
int ifa_model_set_stream(ifa_model *m, ifa_stream stream);

/* ======================================================================== */
/* Collectives of the multi-GPU partitions (RCCL over xGMI; csrc/ifa_comm.hip) */
/* -- what GpuInferenceWorker::DistributeAndMergeTensors / MergeTensors /     */
/* DeviceCopy (src/transformer/inference_worker.cc:2148-2335) and             */
/* GpuInfGlobalData (src/transformer/gpu_inf_global_data.cu:25-199) do with   */
/* host-side spin-waits and serial copies.  Enqueue-only, explicit stream,    */
/* capturable; one communicator per (rank, group).                            */
/* ======================================================================== */
typedef struct ifa_comm ifa_comm;
#define IFA_COMM_ID_BYTES 128
/* one process per GPU: rank 0 makes the id, ships the 128 bytes over any host channel, every rank joins */
int ifa_comm_unique_id(void *id_out_128);
int ifa_comm_init_rank(const void *id_128, int nranks, int rank, int device, ifa_comm **out);
/* one process, one host thread per GPU (the engine facade, like inference_engine.cc:1203-1206): all ranks at once */
int ifa_comm_init_all(const int *device_ids, int n, ifa_comm **comms_out);
/* a device list that names ONE device n times makes an in-process loopback group instead (RCCL refuses two ranks on a
 * device): kernels / copies on that device with a host rendezvous between the rank threads -- host-synchronous, not
 * capturable (ifa_comm_capturable() == 0); for exercising the multi-rank paths on a 1-GPU box */
int ifa_comm_capturable(const ifa_comm *c);
/* identity of the communicator OBJECT (a new one at the same address gets a new serial): what a cached, captured step
 * is keyed on */
unsigned long long ifa_comm_serial(const ifa_comm *c);
/* One-shot all-reduce (csrc/ifa_comm.hip): communicators made by ifa_comm_init_all whose devices can map each other's
 * memory exchange vectors of <= 64 KB directly (push into peer inboxes + epoch flags, sum in rank order in half: the
 * arithmetic of MergeTensors, inference_worker.cc:2197-2260) instead of a ring collective -- one launch per rank, no host
 * rendezvous.  ifa_comm_oneshot: 1 if this communicator does; ifa_comm_set_oneshot(c, 0) keeps RCCL for every size;
 * ifa_comm_status: non-zero if a wait inside a one-shot all-reduce of this rank gave up (2 s). */
int ifa_comm_oneshot(const ifa_comm *c);
/* One process per rank (ifa_comm_init_rank): export allocates this rank's inbox / flags and writes their two IPC handles
 * (IFA_ONESHOT_HANDLE_BYTES); the caller gathers all ranks' handles in rank order over the channel that carried the
 * communicator id; import maps the peers' buffers (hipIpcOpenMemHandle) -- ifa_comm_oneshot(c) is 1 afterwards. */
#define IFA_ONESHOT_HANDLE_BYTES 128
int ifa_comm_oneshot_export(ifa_comm *c, void *handle_out_128);
int ifa_comm_oneshot_import(ifa_comm *c, const void *handles_all_ranks);
int ifa_comm_set_oneshot(ifa_comm *c, int on);
int ifa_comm_status(ifa_comm *c);
/* Wake every rank blocked in (or later entering) a collective of this communicator with an error: called by the rank
 * that failed, or by whoever supervises the ranks (ncclCommAbort, inference_worker.cc has no counterpart: the reference
 * deadlocks its worker threads in this case).  The communicator can only be destroyed afterwards. */
int ifa_comm_abort(ifa_comm *c);
int ifa_comm_destroy(ifa_comm *c);
int ifa_comm_rank(const ifa_comm *c);
int ifa_comm_size(const ifa_comm *c);
/* one host thread issuing the calls of several ranks brackets them with group_start / group_end */
int ifa_comm_group_start(void);
int ifa_comm_group_end(void);
/* BY_TENSOR merge: element-wise sum of the ranks' partial [count] F16 vectors (in place allowed) */
int ifa_allreduce_sum_f16(ifa_comm *c, const void *send_f16, void *recv_f16, size_t count, ifa_stream stream);
/* recv = the ranks' `bytes_per_rank` blocks in rank order (distributed argmax over a vocabulary-sharded lm_head) */
int ifa_allgather(ifa_comm *c, const void *send, void *recv, size_t bytes_per_rank, ifa_stream stream);
int ifa_broadcast(ifa_comm *c, void *buf, size_t bytes, int root, ifa_stream stream);
/* BY_LAYER hand-over of the [T][dim] F16 layer output between device groups (DeviceCopy, :2300-2335) */
int ifa_send(ifa_comm *c, const void *buf, size_t bytes, int peer, ifa_stream stream);
int ifa_recv(ifa_comm *c, void *buf, size_t bytes, int peer, ifa_stream stream);

/* ---- tensor-parallel decode (BY_TENSOR partition, src/transformer/network_builder.cc:1594-1686):
 * the worker holds heads/tp_size heads, kv_heads/tp_size KV heads and ffn/tp_size FFN rows; the
 * caller sums the two partial [dim] F16 vectors per layer over the group exactly where the
 * reference calls DistributeAndMergeTensors (inference_worker.cc:1378-1391, :1882-1895).
 * All calls only enqueue work on the worker's stream.
 *   begin(token,pos)            token < 0 / pos < 0: keep the id / position already in the device state
 *   attn(l, partial)            norm + QKV + attention + Wo product (no bias/residual)
 *   post_attn(l, reduced)       + bias, + residual
 *   ffn(l, partial)             norm + W1/W3 + act + W2 product
 *   post_ffn(l, reduced)        + bias, + residual -> next layer input
 *   logits(shard_out)           final norm + this rank's vocabulary rows of lm_head
 *   set_token(dev_ptr)          next token id from device memory (after the distributed argmax); advances the
 *                               device-side position, so begin(-1,-1) ... set_token() is replayable as a hipGraph */
int ifa_model_tp_begin(ifa_model *m, int token, int pos);
/* BY_LAYER / HYBRID partition (MultiGpuStrategy, src/transformer/model.h:61-66; layer ranges per device group:
 * NetworkBuilder::SplitGpuLayers, network_builder.cc:2094-2118): a worker that holds a layer range only starts its
 * step from the previous group's output instead of an embedding row, and hands its last layer's output on.
 *   begin_hidden(x, pos)   layer input from device memory ([dim] F16); pos < 0 keeps the device-side position
 *   hidden(x_out)          copy of the current layer input/output vector (after the last local layer) */
int ifa_model_tp_begin_hidden(ifa_model *m, const void *x_f16, int pos);
int ifa_model_tp_hidden(ifa_model *m, void *x_out_f16);
int ifa_model_tp_attn(ifa_model *m, int layer, void *partial_out_f16);
int ifa_model_tp_post_attn(ifa_model *m, int layer, const void *reduced_f16);
int ifa_model_tp_ffn(ifa_model *m, int layer, void *partial_out_f16);
int ifa_model_tp_post_ffn(ifa_model *m, int layer, const void *reduced_f16);
int ifa_model_tp_logits(ifa_model *m, void *logits_shard_out_f16);
int ifa_model_tp_set_token(ifa_model *m, const int *token_dev);
/* The whole multi-GPU greedy decode from C: the segments above + the collectives of csrc/ifa_comm.hip on the worker's
 * stream, a distributed argmax over the vocabulary-sharded lm_head, token / position fed back in device memory; the step
 * is captured once as a hipGraph (tensor-parallel groups) and replayed per token.  Every rank calls it with the same
 * arguments (one host thread or process per GPU).  out_tokens_host[n_steps]: the generated ids on every rank. */
typedef struct {
    ifa_comm *tp;          /* this worker's tensor-parallel group (NULL / size 1: nothing to merge) */
    ifa_comm *world;       /* all ranks of the job: hand-over between layer groups + token broadcast (n_stages > 1) */
    int stage, n_stages;   /* BY_LAYER / HYBRID: this worker's device group, number of groups (1 = BY_TENSOR only) */
    int prev_rank, next_rank, token_src;   /* ranks in `world`; -1 = none */
    int vocab_offset;      /* first vocabulary row of this rank's lm_head shard */
    int force_collectives; /* issue the collectives even in a group of one (plumbing check on a 1-GPU box) */
} ifa_tp_topology;
int ifa_model_tp_decode(ifa_model *m, const ifa_tp_topology *topo, int first_token, int start_pos, int n_steps,
                        int *out_tokens_host, float *elapsed_ms);
/* One Infer() step of a query over the partition: n_tokens new tokens at [start_pos, start_pos + n_tokens) fed through
 * the partition: n_tokens > 1 as ONE T > 1 step (row-sliced MFMA GEMMs, [T][dim] merges after wo and w2, [T][dim]
 * hand-over between layer groups), a single token through the decode path; *next_token_host = greedy next token of the
 * last one (every rank).
 * logits_shard_out_dev (nullable; last device group): this rank's lm_head rows of every token, [n_tokens][rows] F16. */
int ifa_model_tp_prefill(ifa_model *m, const ifa_tp_topology *topo, const int *tokens_host, int n_tokens, int start_pos,
                         void *logits_shard_out_dev, int *next_token_host);
/* ifa_model_decode_batch over a tensor-parallel group (one new token for each of n queries; merges over [n][dim], one
 * distributed argmax per row); logits_shard_out_dev: optional [n][this rank's lm_head rows] F16 */
int ifa_model_tp_decode_batch(ifa_model *m, const ifa_tp_topology *topo, int n, const int *tokens_host, const int *positions_host,
                              const int *kv_slots_host, int *next_tokens_host, void *logits_shard_out_dev);
/* reference-layout copy of a loaded tensor (device pointer); returns 1 if the tensor is not set */
int ifa_model_get_tensor(ifa_model *m, int layer, int tensor_id, int *dtype, void **dptr, size_t *rows, size_t *cols);
/* the same for W1 / W2 / W3 of expert `expert` of a mixture-of-experts layer */
int ifa_model_get_expert_tensor(ifa_model *m, int layer, int expert, int tensor_id, int *dtype, void **dptr, size_t *rows, size_t *cols);
/* Average duration (HIP events on the worker's stream) of `iters` back-to-back
 * launches of one fused decode kernel, rotating over the layers' weights:
 * which = 0 qkv, 1 attention, 2 wo, 3 ffn w1/w3, 4 w2, 5 lm_head.  For bench.py's roofline. */
int ifa_model_time_kernel(ifa_model *m, int which, int iters, float *avg_us);

/* The decode route plan (csrc/ifa_decode_route.h, DESIGN.md "Decode route plan"): which attention launch a decode step runs, with
 * which kernel instance.  Host-only, no GPU needed.  facts[22], in the order of DecRouteFacts: head_dim, heads, kv_heads, max_ctx,
 * kv_q8, reach, attn_split_ctx, attn_nsplits, attn_kt, attn_unload, fuse_attn, fuse_ffn, attn_q8, tail_layers_ok, gk, rw,
 * chain_level, have_attq, waits, num_cus, visible_cus, own_launches.  out[14], in the order of DecRoute: kind (0 one workgroup per
 * head, 1 keys split over workgroups, 2 tail of the fused QKV launch), nsplits, pb, kt, ul, gk, rw, chain, split_threshold, split,
 * lds_attn, lds_scores, lds_pv, error. */
int ifa_decode_route_plan(const int *facts, int n_facts, int *out, int n_out);
/* The plan of the model's last decode / decode_prepare / time_kernel call: out[17] = the 14 values above, then num_cus,
 * visible_cus and waits (1: launches whose workgroups wait for each other are allowed) as the engine sees them now. */
int ifa_model_decode_route(ifa_model *m, int *out, int n_out);

/* The decode GEMV launch plan (csrc/ifa_decode_gemv_plan.h): which fused GEMV instance a launch runs.  Host-only, no GPU needed.
 * facts[8], in the order of DecGemvFacts: dtype (an element type id, or 99 for Q3H_B64T1 streamed in its native 32-byte form: option
 * q3h_native), epi (0 plain, 1 residual, 2 gated pair, 3 activation, 4 - 7 the expert epilogues), norm
 * (0 none, 1 RMS-norm prologue, 2 the activation arrives quantised), x_add, cols, total_rows (gated: row pairs), num_cus, rpw (the
 * rpw_* option).  out[13], in the order of DecGemvPlan: kind (0 none, 1 k_dec_gemv, 2 k_dec_gemv_long, 3 k_dec_gemv_h), nj, nchunk,
 * njl, rw, threads, np, grid, waves, npass, partial (the last pass is short), lds, error (0 ok, 1 dtype, 2 columns, 3 more than 4
 * chunks / 32768 columns, 4 too many blocks per lane for a normalised / gated input, 5 packed launch scalars, 6 no such instance). */
int ifa_decode_gemv_plan(const int *facts, int n_facts, int *out, int n_out);
/* The same for the launch of one role (0 qkv, 1 wo, 2 w1 / w3, 3 w2) of a layer as the engine would enqueue it now: out[21] = the 13
 * values above, then single (0: the step would not run this launch on its own: the fused QKV + attention tail, the chained FFN
 * launch or the op-by-op step takes its place), dtype, epi, norm, cols, total_rows, num_cus, launches (3: q / k / v of different
 * formats get one launch each, the plan is wq's). */
int ifa_model_gemv_plan(ifa_model *m, int layer, int role, int *out, int n_out);

/* The prompt and batched-step route plans (csrc/ifa_prompt_route.h, DESIGN.md "Prompt route plan"): which kernels the linears of a
 * prompt's / a batched step's layers go through, from which copy of the weights, and what is built first.  Host-only, no GPU needed.
 * Prompt: facts[19], in the order of PromptRouteFacts: T, exact_order, perf_stat, prefill_chunk, prefill_mid, prefill_mid_max,
 * prefill_big, prefill_big_min, prefill_res_mid, rows_mo, gemm_rows, batch_fused, gemm_splitk, rows_kparts, topo, experts, rows_layers
 * (0 no, 1 from MO copies only, 2 from the tiled layout too), big_layers, mid_shapes.  out[22], in the order of PromptRoute: kind (0 exact
 * order, 1 op by op, 2 rows GEMM, 3 mid-length GEMM, 4 large tiles), first_pass, norm_fused, res_mid, then (kernel, src, mo, no_waits) of
 * wq | wk | wv, wo, w1 / w3 and w2 (kernel 0 rows / 1 mid / 2 large tiles; src 0 tiled / 1 MO copy / 2 x32 copy or reference rows), need_mo
 * (2: after the x32 copies), need_x32.
 * Batched step: facts[13], in the order of BatchRouteFacts: n, exact_order, may_chunk, rows_mo, gemm_rows, batch_fused, rows_kparts,
 * batch_graph, graph, topo, rows_layers, has_moe, logits_out.  out[9], in the order of BatchRoute: kind (0 exact order, 1 op by op,
 * 2 fused), chunk, norm_fused, captured, (kernel, src, mo, no_waits) of every product, need_mo. */
int ifa_prompt_route_plan(const int *facts, int n_facts, int *out, int n_out);
int ifa_batch_route_plan(const int *facts, int n_facts, int *out, int n_out);
/* The route of the model's last prompt call (ifa_model_forward and what runs through it), out[22] as above; a prompt of two passes
 * shows first_pass 32 and the first pass's route.  Plans nothing, allocates nothing. */
int ifa_model_prompt_route(ifa_model *m, int *out, int n_out);

/* The launch plans of the prompt GEMMs (csrc/ifa_gemm_plan.h, DESIGN.md "Prompt GEMM launch plans").  Host-only, no GPU needed.
 * k_gemm_mid: facts[18], in the order of GemmMidFacts: T, nsets, rows0, rows1, rows2, nblk (32-weight blocks per row), epi (0 plain,
 * 1 residual, 2 gated pair), num_cus, no_waits, waits_on, then the measurement settings (0 = default) max_parts, ta, min_steps, two_per_cu,
 * no_glu_split, then mo, has_w1, ld_or (the strides read, or-ed).  out[25], in the order of GemmMidPlan: error (0 ok, 1 not an MO copy,
 * 2 shape, 3 rows % 16, 4 gated pair without one set and W3, 5 a stride % 8), ta, tiles_m, tiles_n, tile0[4], ksteps, n_try, then
 * parts[5], grid[5], lds[5] of the candidates in the order they are tried (the next one when a waiting grid cannot be resident).
 * k_gemm_big: facts[14], in the order of GemmBigFacts: T, nsets, rows0, rows1, rows2, nblk (blocks per row), dtype, epi, tiles_bits (the
 * value of ifa_gemm_big_tiles), num_cus, no_waits, waits_on, has_w1, ld_or.  out[23], in the order of GemmBigPlan: error (0 ok, 1 format,
 * 2 shape, 3 fused epilogue on another format than Q4_B32T1A / B, 4 gated pair, 5 rows % 8, 6 a stride % 8), pick (1 256 x 256, 2 128 x
 * 256, 3 128 x 128, 4 - 6 the small tiles), stream_k, n_launch, then (bm, bn, waves, tn0, tn_count, tiles_m, lds) of the two launches,
 * full_n, rem_n, n_try, ks[2] (parts of K in the order they are tried). */
int ifa_gemm_mid_plan(const int *facts, int n_facts, int *out, int n_out);
int ifa_gemm_big_plan(const int *facts, int n_facts, int *out, int n_out);
/* The launch plan of the rows GEMM (k_gemm_rows_mfma; csrc/ifa_gemm_rows_plan.h, DESIGN.md "Rows GEMM launch plan").  Host-only.
 * facts[17], in the order of GemmRowsFacts: T, nsets, rows0, rows1, rows2, nblk, epi (0 plain, 1 residual, 2 gated pair), norm, mo, has_w1,
 * no_waits, waits_on, num_cus, visible_cus, then the settings (0 = default) wgs_per_cu, kparts_off, kparts_min.  out[22], in the order of
 * GemmRowsPlan: error (0 ok, 1 shape, 2 norm prologue, 3 gated pair, 4 rows, 5 byte offsets past 32 bits, 6 no instance for the epilogue /
 * norm), total_rows, ntiles, tx (rows staged), ch (1 one chunk, 0 chunk loop, 2 whole rows), chunk_cols, nchunk, n_try, then per attempt in
 * the order they are tried (kparts, kpm, tiles per workgroup or group, groups, grid, lds, scratch bytes): K parts first where they apply,
 * the plain launch (kparts 0) last. */
int ifa_gemm_rows_plan(const int *facts, int n_facts, int *out, int n_out);
/* The last rows GEMM launches of this process, oldest first; reading clears them.  out[2 + 8 x 23]: out[0] records that follow (at most 8),
 * out[1] launches since the last read, then per record: T, total_rows, nblk, epi, norm, mo, tx, ch, nchunk, n_try, attempt (index of the
 * attempt that ran), the attempt's seven plan fields, and -- attempt > 0: the K-parts attempt was declined -- what the residency test saw:
 * declined_grid, occupancy (workgroups per CU; -1 not asked), visible_cus, waits_on, err_word (the wait-error word exists).  A captured step
 * records when it is captured, not when it is replayed. */
int ifa_gemm_rows_launches(int *out, int n_out);
/* Test hook of that record's ring, host only: rec[23] is pushed as a launch would push it; count_before >= 0 sets the count of launches
 * since the last read first (the count saturates at 2^31 - 1; the slot index stays in 0 .. 7). */
int ifa_debug_gemm_rows_record(const int *rec, int n_rec, int count_before);

/* The plan of a mixture-of-experts layer over the T rows of a step (csrc/ifa_moe_plan.h, DESIGN.md "MoE layer plan").  Host-only, no GPU
 * needed.  facts[28], in the order of MoeFacts: T, experts, top_k, dim, ffn (rows of an expert's W1), w_dtype, w_ax8, w_q4, full_quant_gemv,
 * norm_kind, gate_f16, gate_cols_match, has_ffn_norm, experts_uniform, have_table, have_table_aos, have_table_mo (the pointer tables the
 * layer holds: tiled, reference layout, MO copies), the options moe_device, moe_router_fused, moe_singles, moe_overlap, gemm_rows, rows_mo,
 * the launchers' predicates rows_use_mfma, rows_mfma_ok, rows_q4_ok, singles_ok, and caller_norm (the caller hands over the rows before the
 * FFN norm and leaves norm and residual to the layer: the fused batched step).  out[14], in the order of MoePlan: kind (0 host-routed,
 * 1 device-routed grouped launches, 2 device-routed with the single-row experts as two launches), router (0 norm / gate / softmax / top-k
 * launches, 1 one launch; T = 1: the router of the fused decode step), device_ok, cap (T x top_k), tile_rows, small_max, max_tiles,
 * max_singles, max_smalls, rows_kernel, rows_mfma, smalls_mo, side_stream (the singles' launches fork to a second stream), host_sync (the
 * layer synchronises the stream: never captured).  A host-routed layer has the fields from tile_rows to side_stream at 0. */
int ifa_moe_plan(const int *facts, int n_facts, int *out, int n_out);
/* The plan the model would follow for an MoE layer over T rows NOW (its options, the tables it has built so far), out[14] as above.
 * IFA_ERR_ARG for a layer without experts.  Plans only: launches and allocates nothing. */
int ifa_model_moe_plan(ifa_model *m, int layer, int T, int caller_norm, int *out, int n_out);

/* The pooled rows ONE step of a pool call serves (csrc/ifa_pool_rows_plan.h, DESIGN.md "Step tails").  Host-only, no GPU needed.
 * rows_sel[n_sel]: the call's pooled rows, strictly ascending indices into its rows; adj[n_sel] or NULL: state slot of pooled row j, < 0
 * raw (ifa_model_pool_adjust); cursor: pooled rows the call's earlier steps have served; the step runs the call's rows
 * [chunk0, chunk0 + n_rows).  runs_out[cap_runs][3] takes (ja, jb, armed) per run of pooled rows [ja, jb): maximal within the step, all
 * armed or all raw, in order; *n_runs their number; *cursor_out the cursor behind the step. */
int ifa_pool_rows_plan(const int *rows_sel, const int *adj, int n_sel, int cursor, int chunk0, int n_rows, int *runs_out, int cap_runs,
                       int *n_runs, int *cursor_out);

#ifdef __cplusplus
}
#endif
#endif /* INFERFLOW_AMD_H_ */
