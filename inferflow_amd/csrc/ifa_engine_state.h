// ifa_engine_state.h -- the per-device worker's state (struct ifa_model: tensors, scratch, captured steps, options) and the
// functions its translation units share.  The worker is the MI355X counterpart of GpuInferenceWorker
// (src/transformer/inference_worker.cc:234-340); it is split by what a unit does, not by layer:
//   ifa_engine.hip          model life cycle: create / set_tensor / finalize / KV slots / options / buffers (the C ABI's ifa_model_* basics)
//   ifa_engine_decode.hip   the fused batch-1 decode step: launch parameters of every fused kernel, graph capture, ifa_model_decode
//   ifa_engine_forward.hip  prompts and batched steps: op-by-op layer, the four-launch prompt routes, batched steps, ifa_model_forward
//   ifa_engine_moe.hip      mixture of experts: the router on the device, grouped expert launches of a batch, the host-routed fallback
//   ifa_engine_exact.hip    option exact_order: single-token steps in the reference kernels' summation order (parity instrument)
//   ifa_engine_tp.hip       tensor / layer partitions: per-seam entry points and the multi-GPU step driven from C
//   ifa_kv_copy.hip         cache rows from one query slot to another in one launch (the engine's prompt prefix cache)
//   ifa_decode_draft_kv.hip the draft step: n rows of ONE slot in one batched step (ifa_model_decode_draft; the engine's lookup decoding)
//
// Worker memory.  Every device or pinned block the worker owns is a DevBuf / PinBuf / DevPin member (ifa_buf.h, ifa_buf_hip.h) of
// the struct that uses it: it is freed when its owner goes -- `delete m`, a Tensor assigned over, a KvSlot dropped -- and by nothing
// else, so no unit keeps a free list.  The members read as plain pointers.  Growth is all-or-nothing: a unit allocates the new
// blocks into locals (or Staged::reserve / Buf::alloc, which hold everything or nothing with capacity 0) and installs them only
// when every allocation has succeeded; a failed growth leaves either the old state or an empty one the next call rebuilds, never a
// size over freed memory.  Captured steps hold buffer addresses: whoever moves a buffer calls drop_graphs().
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#include "ifa_host.h"
#include "ifa_buf_hip.h"
#include "ifa_decode_kernels.h"
#include "ifa_decode_attn.h"
#include "ifa_decode_gemv.h"
#include "ifa_moe.h"
#include "ifa_gemm_rows_mfma.h"
#include "ifa_gemm_big.h"
#include "ifa_decode_lmhead_tail.h"
#include "ifa_decode_singles.h"
#include "ifa_decode_qkv_attn.h"
#include "ifa_decode_chain.h"
#include "ifa_prompt_route.h"
#include "ifa_moe_plan.h"
#include "ifa_pool_rows_plan.h"

using namespace ifa;

namespace ifae {


enum { T_EMBD = 0, T_OUT_NORM = 1, T_OUT_NORM_B = 2, T_LM_HEAD = 3,
       T_ATTN_NORM = 10, T_ATTN_NORM_B = 11, T_WQ = 12, T_WK = 13, T_WV = 14, T_WO = 15,
       T_FFN_NORM = 16, T_FFN_NORM_B = 17, T_W1 = 18, T_W2 = 19, T_W3 = 20, T_MOE_GATE = 21,
       T_WQ_B = 22, T_WK_B = 23, T_WV_B = 24, T_WO_B = 25, T_W1_B = 26, T_W2_B = 27, T_W3_B = 28,
       T_ATTN_POST_NORM = 29, T_ATTN_POST_NORM_B = 30, T_FFN_POST_NORM = 31, T_FFN_POST_NORM_B = 32,      // self_attn.post_norm / feed_forward.post_norm (model.h:168-276)
       T_MAX = 36 };

struct Tensor {
    int dtype = -1;
    DevBuf<void> data;       // reference layout (AoS blocks / F16), engine-owned
    DevBuf<void> tiled;      // row-local plane layout for the fused kernels (or null)
    DevBuf<void> mo;         // MFMA-operand-order copy for the small-batch rows GEMM (ifa_gemm_rows_mfma.h), built on first use
    DevBuf<void> q3hn;       // Q3H_B64T1: the values at the format's native 32 bytes per block for the decode GEMVs (option q3h_native, built on first use)
    DevBuf<void> x32;        // 64-weight nibble formats: the same values as Q4_B32T1A reference-layout blocks, for the large-tile prefill GEMM
    size_t rows = 0, cols = 0;
    bool present() const { return data != nullptr; }
};

struct Layer {
    Tensor t[T_MAX];
    std::vector<Tensor> experts;   // [expert][3]: w1, w2, w3 (MoE layers)
    DevBuf<void *> moe_table;      // device: [expert][4] tiled pointers {w1, w3, w2, -} for the fused decode kernels
    DevBuf<void *> moe_table_aos;  // device: [expert][3] reference-layout pointers {w1, w2, w3} for the grouped T > 1 launches
    DevBuf<void *> moe_table_mo;   // device: [expert][4] MO copies {w1, w3, w2, -} for the experts with 2..8 rows of a batched step (ensure_mo)
    DevBuf<void> kcache, vcache;
};

// Activation scratch, sized for scratch_tokens rows by ensure_scratch (which builds a new set and move-assigns it: all or nothing).
// dqkv, attq and moe_route are allocated once, bqkv / brope once a step of <= 32 rows asks; those keep their address over a growth.
struct Scratch {
    DevBuf<half_t> x, x2, xn, hn, q, k, v;
    DevBuf<half_t> dqkv;        // the decode step's q | k | v vector as ONE buffer (k_dec_attn addresses k and v from q's pointer)
    DevBuf<half_t> bqkv;        // fused batched step: [32 queries][q | k | v]
    DevBuf<float> brope;        // fused batched step: [32 queries][head_dim] (cos, sin) pairs
    DevBuf<half_t> att, a, f, t1, t2, logits;
    DevBuf<uint8_t> xq;
    DevBuf<int8_t> attq;           // XqImage of the attention output (Q8_B32T2), written by the fused attention kernels for the Wo GEMV
    DevBuf<half_t> moe_gate, moe_out;     // MoE: router probabilities [T][experts], one expert's output rows
    DevBuf<half_t> moe_in, moe_wdev;      // MoE: one expert's gathered input rows; per-row weights
    DevBuf<int> moe_route;                // device: fused decode routing, [0..7] expert ids, halfs at byte 32: weights
    DevBuf<int> moe_idx; PinBuf<void> moe_pin;     // MoE: row lists of all experts, back to back (device / pinned staging)
    // MoE over T > 1 rows without the host (moe_ffn_device): routing, lists, gathered rows of ALL experts at once
    DevBuf<int> moe_sel, moe_epos, moe_counts;
    DevBuf<half_t> moe_selw, moe_g1, moe_g3, moe_gin, moe_gout;
    DevBuf<uint8_t> moe_xq_in, moe_xq_mid;
    DevBuf<void> moe_tiles, moe_singles, moe_smalls;
    DevBuf<int> tokens_dev;
    DevBuf<half_t> pn;             // [tokens][dim] scratch of the post norms
};


// ---- Step tails: what a step does behind its logits and in front of its one synchronisation ("Step tails").  The entry
// point builds a StepTail on its stack and hands it down through decode_impl / forward_ops / forward_exact / forward_batch /
// enqueue_fused_step; each of them calls tail_enqueue() at one place.  Nothing of a tail lives in the model: what a call of several
// steps has served so far is the entry point's TailCursor.
struct SampledCall { const ifa_sample_params *p = nullptr; unsigned long long *rng = nullptr; int state_slot = -1; };
enum TailKind {
    TAIL_NONE = 0,         // the greedy id only
    TAIL_POOL,             // candidate pools of the wanted rows (+ their log-sum-exp), one copy of the block into pinned staging
    TAIL_SCORE,            // log-sum-exp + target logit of every row of a prompt; behind the last row one copy into pinned staging
    TAIL_DRAFT_VERIFY,     // the n rows of a draft step: [processors ->] pools -> the chained draws (k_sample_verify) -> one copy
    TAIL_SAMPLED,          // INSIDE the fused step, captured with it: lm_head -> [processors ->] pool -> draw + state advance
    TAIL_FED               // a batched step of a device-fed call: only enqueues -- no copy back, no synchronisation; its caller feeds
};
struct StepTail {
    TailKind kind = TAIL_NONE;
    int k = 0;                             // POOL / DRAFT_VERIFY / SAMPLED: pool length
    int n = 0;                             // POOL: pooled rows (1 for a single-query step); SCORE: rows of the prompt (targets on the device)
    const int *rows_sel = nullptr;         // POOL, batched step: ascending row indices (host); null: the step's last row
    bool lse = false;                      // POOL: the rows' log-sum-exp ride in the block (option pool_lse)
    const int *adj = nullptr;              // POOL: logit processors, [n] state slot of pooled row j, -1 raw (the entry point's array); null: none
    bool armed = false;                    // DRAFT_VERIFY / SAMPLED: the logit processors of the call's state slot run first
    const SampledCall *sampled = nullptr;  // SAMPLED: what the call writes into samp_blk
    bool fed_first = false;                // FED: the call's first step (its tables go up in front of the replay)
};
struct TailCursor {
    int done = 0;                          // POOL: pooled rows whose launches are enqueued; SCORE: rows
    int chunk0 = 0; bool last_chunk = true;      // a batched step taken as several steps: first row of this one / it is the last
};

// the result block of the pool steps: counts [n_sel] | (with_lse: lse [n_sel] |) ids [n_sel][k] | F16 bits [n_sel][k]
struct PoolBlock { int *counts; float *lse; int *ids; uint16_t *vals; size_t bytes; };
static inline PoolBlock pool_block(void *base, int n_sel, int k, bool with_lse)
{
    PoolBlock B;
    B.counts = (int *)base;
    B.lse = with_lse ? (float *)(B.counts + n_sel) : nullptr;
    B.ids = B.counts + (with_lse ? 2 : 1) * n_sel;
    B.vals = (uint16_t *)(B.ids + (size_t)n_sel * k);
    B.bytes = (size_t)n_sel * (with_lse ? 8 : 4) + (size_t)n_sel * (size_t)k * 6;
    return B;
}

// The call blocks in device memory (+ pinned twin): what differs from call to call and is no kernel argument of a captured launch.
// Sampled decode: all of it goes up in front of the first step, [rng, end) comes back behind the last.
struct SampBlk { ifa_sample_params p; unsigned long long rng; int slot, err, token, index, pad[4]; };
static_assert(offsetof(SampBlk, rng) % 8 == 0 && offsetof(SampBlk, slot) == offsetof(SampBlk, rng) + 8, "SampBlk: the generator word is aligned, what comes back is contiguous");
// Sampled draft step: all of it goes up, [rng, back_end) comes back.
struct DraftBlk { ifa_sample_params p; int slot, pad0, draft[8]; unsigned long long rng; int n_out, err, tokens[8], back_end[4]; };
static_assert(offsetof(DraftBlk, rng) % 8 == 0 && offsetof(DraftBlk, n_out) == offsetof(DraftBlk, rng) + 8 && offsetof(DraftBlk, back_end) == offsetof(DraftBlk, tokens) + 32,
              "DraftBlk: the generator word is aligned, what comes back is contiguous");
// Device-fed batched steps: [rows, ring) and [params, end) go up (the ring is written by the device); [rows, ring + n_steps * n) comes back.
struct BatchStepsBlk {
    ifa_batch_feed_row rows[IFA_BATCH_ROWS_MAX];
    int step, err, draw_err, pad;
    int ring[IFA_BATCH_STEPS_MAX * IFA_BATCH_ROWS_MAX];
    ifa_sample_params params[IFA_BATCH_ROWS_MAX];
    unsigned long long rng[IFA_BATCH_ROWS_MAX];
    int pool_len[IFA_BATCH_ROWS_MAX], drawn[IFA_BATCH_ROWS_MAX], index[IFA_BATCH_ROWS_MAX], pair_slot[IFA_BATCH_ROWS_MAX], pair_tok[IFA_BATCH_ROWS_MAX];
};
static_assert(offsetof(BatchStepsBlk, rng) % 8 == 0 && offsetof(BatchStepsBlk, ring) == offsetof(BatchStepsBlk, step) + 16 && sizeof(ifa_batch_feed_row) % 8 == 0
              && offsetof(BatchStepsBlk, params) == offsetof(BatchStepsBlk, ring) + sizeof(int) * IFA_BATCH_STEPS_MAX * IFA_BATCH_ROWS_MAX,
              "BatchStepsBlk: the 8-byte words are aligned, what comes back is contiguous");

} // namespace ifae
using namespace ifae;

struct ifa_model : Scratch {
    ifa_model_config cfg;
    std::vector<Layer> layers;
    Tensor g[10];
    hipStream_t stream = nullptr;
    // side stream + fork / join events of the batched MoE step: the single-row experts run next to the small groups (both stream
    // expert matrices nobody else reads and neither saturates the memory system alone); created on first use
    hipStream_t side_stream = nullptr; Event ev_fork, ev_join; int opt_moe_overlap = 1;
    bool own_stream = true;
    bool finalized = false;
    int opt_moe_device = 1;
    DevBuf<int> state;             // device: see k_dec_gather
    DevBuf<float> rope_tab;        // device: [head_dim/2][2]
    DevBuf<long long> trace;       // device: [2048][8] optional kernel phase stamps
    int opt_trace = 0, opt_bench_mode = 0, opt_touch_stride = 65536;
    int opt_time_pos = -1;               // ifa_model_time_kernel: position of the timed launches (-1: 64); the route is the last call's
    PinBuf<int> host_pinned;       // pinned staging for state / tokens
    int scratch_tokens = 0;
    size_t kv_row_bytes = 0;
    // decode graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    // the same step captured opt_graph_steps times in a row (option graph_steps, default 1 = off): a replay boundary costs ~8.6 us
    // against ~1.5 us between two launches inside a graph (rocprofv3 trace of the bench) -- but replays of 4 / 8 / 16 steps measured
    // SLOWER per token than single steps (1.2514 / 1.2524 / 1.2502 ms against 1.2427: profiles/r04_ab_options.log), so it stays opt-in
    hipGraph_t graph_n = nullptr; hipGraphExec_t graph_exec_n = nullptr; int graph_n_steps = 0, opt_graph_steps = 1;
    // tensor parallelism: a seam's "layer input + merged product (+ bias)" waiting to be formed in the prologue of the
    // GEMV that consumes it (instead of one or two tiny add kernels per seam)
    struct PendingAdd { const half_t *x = nullptr, *add = nullptr, *bias = nullptr; half_t *out = nullptr; bool on = false; } pend;
    int opt_tp_fuse_add = 1;
    // dynamic batching tables (forward_batch)
    DevPin<void> batch_tab;
    std::map<int, hipGraphExec_t> batch_graphs;      // captured batched step per batch size (dense models)
    std::map<int, hipGraphExec_t> draft_graphs;      // captured draft step (ifa_model_decode_draft: n rows of ONE slot) per row count
    // Device-fed batched steps (ifa_model_decode_batch_steps, ifa_engine_batch_steps.hip).  fed_graphs: the batched step per row
    // count WITHOUT the table upload in front and the copy of the greedy ids behind it -- the tables are uploaded once per call and
    // advanced on the device (csrc/ifa_batch_feed.hip).  bs_blk: the call's per-row feed state, parameters, generator words, token
    // ring and error word in device memory (+ pinned twin), written by the call like samp_blk.
    std::map<int, hipGraphExec_t> fed_graphs;
    DevPin<BatchStepsBlk> bs_blk;
    // long-context decode attention (keys split over workgroups): workspace, switch and the context it starts at
    DecAttnSplitWs attn_ws = {nullptr, nullptr, nullptr, 8};      // (what the kernels take: filled from the three owners below; nsplits per launch from the route)
    DevBuf<half_t> attn_ws_S; DevBuf<float> attn_ws_lmax, attn_ws_opart;
    int opt_attn_unload = 1;       // 1 (default): in the 256-row bucket the heads' workgroups of the fused QKV + attention launch take no weight rows (UL kernels)
    int opt_attn_nsplits = 0;      // > 0: splits per head whatever the context (measurement)
    // What the decode step of the last planned call runs (ifa_decode_route.h: the attention launch, its kernel instance, the chained
    // FFN launch) and the reach it was planned for; the captured steps hold it (decode_route_ready)
    DecRoute route; int route_reach = 256;
    PromptRoute prompt_route;      // what the last prompt call ran (ifa_prompt_route.h, prompt_route_ready)
    // attention as the tail of the QKV launch (ifa_decode_qkv_attn.h): granules [layers][(heads + 2 kv_heads) * head_dim], the
    // decode-call counter the tags are built from, its own error word
    int opt_fuse_attn = 1, opt_fuse_attn_timeout_us = 20000;
    DevBuf<unsigned long long> qa_gran;
    DevBuf<unsigned> qa_call, qa_err; unsigned qa_calls = 0;
    // consecutive GEMV ops of a layer as ONE launch with the next op's rows requested before the hand-off (ifa_decode_chain.h):
    // option fuse_ffn = 1: W1 | W3 -> W2; 2: Wo -> W1 | W3 -> W2 (route.chain = what the captured step uses).  Granules [layers][dim + ffn].
    int opt_fuse_ffn = 0, opt_chain_late_w2 = 0;
    int opt_q3h_native = 0;          // Q3H_B64T1 linears of the dense FFN and Wo streamed at 32 instead of 36 bytes per block (A / B: profiles/r06_q3h_native_ab.log)
    // Per-phase times in the reference's key space (InferencePerfStat, GpuInferenceWorker::UpdatePerfStat, inference_worker.cc:2670-2697:
    // (layer + 1) * 10000 + phase, the whole layer under + 0 for layers 0..5, the phases of layer 0 -- layer_idx_for_study_ -- under
    // + 10 / 30 / 50 / 60 / 90 / 300 / 700 / 710 / 730 / 750 / 760 / 780 / 800, the output stage under 1000009, the embedding rows under 1).
    // Option perf_stat = 1: steps and prompts take the op-by-op layer (one launch per reference op) with a HIP event pair around every
    // phase; ifa_model_perf_stat reads the accumulated milliseconds.  The reference times the host side of the launches (TaskMonitor);
    // these are device times of the same spans.
    int opt_perf_stat = 0;
    struct PerfSpanRec { int key; hipEvent_t e0, e1; };
    std::vector<PerfSpanRec> perf_spans;
    std::vector<hipEvent_t> perf_pool;
    std::map<int, float> perf_map;
    int opt_exact_order = 0;         // single-token steps in the reference kernels' summation order (ifa_engine_exact.hip): bit-identical to the oracle
    DevBuf<float> exact_rope_tab;    // device: [max_ctx][head_dim / 2] (cos, sin) from the host libm, built on the first exact step
    DevBuf<uint32_t> ch_gran, ch_flags;                    // flags [layers][2][CH_FLAGS]
    // the end of the step as one launch (ifa_decode_lmhead_tail.h): lm_head + argmax + state advance + the next step's gather.
    // st_on = what the captured step uses (F16 lm_head with the RMS / no final norm)
    int opt_step_tail = 1, st_on = 0;
    DevBuf<unsigned long long> st_keys; DevBuf<unsigned> st_counter;      // (st_keys.cap(): the lm_head grid the keys serve)
    int opt_attn_kt = 1;      // K rows of the one-workgroup decode attention through the LDS tile
    int opt_attn_split_ctx = -1, opt_batch_graph = 0, opt_gemm_rows = 1, opt_batch_fused = 1, opt_moe_router_fused = 1, opt_prefill_big = 1, opt_rows_mo = 1, opt_moe_singles = 1;
    // independent KV caches ("query slots", one per concurrent query like the reference's per-query
    // LayerKVCache sets): the inactive ones park their cache pointers and captured graph here
    struct KvSlot { std::vector<DevBuf<void>> k, v; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
    std::vector<KvSlot> slots;
    int cur_slot = 0;
    // options
    int opt_attn_q8 = 1;
    // multi-GPU decode driven from C (ifa_model_tp_decode): merge buffers, the distributed argmax's scratch, the captured step
    DevBuf<half_t> tp_a, tp_f, tp_hid, tp_logits;
    DevBuf<float> tp_best, tp_gather;      // (tp_tok.cap(): the rows the distributed-argmax scratch -- these three -- holds)
    DevBuf<int> tp_tok;
    hipGraph_t tp_graph = nullptr;
    hipGraphExec_t tp_graph_exec = nullptr;
    // what the captured multi-GPU step was recorded with: communicator identities and every topology field its launches
    // depend on.  A call with anything else re-captures (a replay would use a stale communicator / offsets).
    struct TpKey {
        unsigned long long tp = 0, world = 0; int tp_size = 0, stage = 0, n_stages = 0, prev = 0, next = 0, src = 0, voff = 0, force = 0, fuse = 0, slot = 0, oneshot = 0;
        bool operator==(const TpKey &o) const { return tp == o.tp && world == o.world && tp_size == o.tp_size && stage == o.stage && n_stages == o.n_stages
                && prev == o.prev && next == o.next && src == o.src && voff == o.voff && force == o.force && fuse == o.fuse && slot == o.slot
                && oneshot == o.oneshot; }      // (oneshot: the captured collectives are the exchange or RCCL -- a switch forces a re-capture)
    } tp_key;
    const ifa_tp_topology *topo = nullptr;     // set by the partition entry points for the duration of a T > 1 / batched step
    // is_attn_post_as_residual (model.h:113, default true): with an attention post-norm, the FFN's residual is the NORMALISED tensor
    int opt_attn_post_as_residual = 1;
    int opt_fused = 1, opt_graph = 1, opt_rpw_qkv = 0, opt_rpw_wo = 0, opt_rpw_ffn = 0, opt_rpw_w2 = 0, opt_rpw_lm = 0;
    int opt_debug_layers = 0;                  // > 0: the decode step runs only the first N layers (tools/debug_engine.py)
    // layer-wise parity tests (tests/test_gpu_layerwise_oracle.py): the fused decode step starts at layer debug_layer0 (with
    // debug_layers = N: layers [layer0, layer0 + N)) and, with debug_hidden_in, takes its input from the buffer "x" as the caller
    // left it instead of gathering the token's embedding row -- the SAME captured launches the bench times, fed the oracle's state
    int opt_debug_layer0 = 0, opt_debug_hidden_in = 0;
    // prompts ABOVE this many tokens take the four large-tile launches per layer (forward_ops on a Big route).  Round 4: 128.  Round 5: 47 -- with
    // four parts of K for the products that offer 32..96 tiles, 64 / 96 / 128 tokens run 5 / 8 / 9 % faster than the op-by-op layer
    // (7 products + 4 element-wise launches), 40 tokens the same (profiles/r05_prompt_lengths.log)
    int opt_prefill_big_min = 47;
    int opt_prefill_chunk = 1;      // prompts of 34..48 tokens as two passes of <= 32 tokens (ifa_model_forward)
    // round 6: prompts of 33 .. prefill_mid_max tokens take the four launches per layer from k_gemm_mid (ifa_gemm_mid.hip: ring of
    // direct-to-LDS stages requested by loader waves, weights dequantised into the MFMA operand registers) when every linear has its
    // operand-order copy; 320..768 tokens 8-9 % faster than the large tiles, 1024 tokens a tie (profiles/r06_prefill_mid_parts.log)
    int opt_prefill_mid = 1, opt_prefill_mid_max = 768;
    int opt_prefill_res_mid = 2048;   // prefill_mid_max + 1 .. this many tokens: wo / w2 still through k_gemm_mid, the other products through the large tiles (0: never)
    int opt_rows_kparts = 1, opt_gemm_splitk = 1;   // 0: never the launches whose workgroups wait for partner workgroups (K parts of the 9..32-row GEMM, split-K halves of the large-tile GEMM)
    int opt_debug_mo_alloc_fail = 0;           // tests: ensure_mo_build fails like an exhausted allocator after its first copy
    // Memory of the step tails (StepTail above; the tails themselves live on the entry points' stacks).
    // Candidate pools (ifa_engine_pool.hip): the result block (PoolBlock), device / pinned.
    DevBuf<unsigned> pool_excl;                // device bitmask of ids the pool never offers (null: none)
    DevPin<void> pool_blk;                     // result block, device / pinned
    DevPin<int> pool_idx;                      // row indices [cap / 2] | state slots of armed rows [cap / 2] (logit processors)
    // Logit processors (ifa_logit_adjust.hip): per KV slot the u32 state row, the f32 bias row and {rep, freq, pres}, allocated for
    // la_slots slots on the first ifa_model_logit_state_reset (regrown, contents kept, when ifa_model_kv_slots has added slots).
    // pool_adj_next: what ifa_model_pool_adjust armed for the next pool call (moved into that call's StepTail at entry, consumed on every
    // way out).  la_adj: the adjusted rows of the last armed step, [rows][vocab] (la_adj_reserve).  la_ring: LA_RING staging blocks of 2 * RING ints (slots | tokens)
    // for ifa_model_logit_state_add, block i guarded by la_ev[i]; reset's prompt / bias staging is la_reset.
    static constexpr int LA_RING = 8;
    DevBuf<unsigned> la_state; DevBuf<float> la_bias, la_params; size_t la_slots = 0;
    DevBuf<half_t> la_adj;
    std::vector<int> pool_adj_next;
    DevPin<int> la_ring; Event la_ev[LA_RING]; bool la_ev_used[LA_RING] = {}; unsigned la_calls = 0;
    DevPin<int> la_reset;
    // option pool_lse = 1: the pool steps also deliver the log-sum-exp of every pooled row (csrc/ifa_logprob.hip; log p = value - lse).
    // The block then reads counts [n_sel] | lse [n_sel] | ids | F16 bits, still one copy; ifa_model_pool_lse hands out the last step's.
    int opt_pool_lse = 0;
    std::vector<float> pool_lse_last;
    DevBuf<float> lse_part;                    // device: (max, sum) pairs of the rows a launch splits over workgroups (LSE_PART_FLOATS)
    // Scoring prompt (ifa_model_forward_score, ifa_engine_score.hip): the targets and the results of its rows
    DevPin<int> score_tgt;                     // [cap] target ids
    DevPin<float> score_out;                   // lse [cap] | target logit [cap]
    // Slot-to-slot copy of cache rows (ifa_model_kv_copy, ifa_kv_copy.hip): the K and V buffers of EVERY slot as one device table
    // [slot][layer: k, v], staged once through kvc_tab.pin on the model's stream and rebuilt only when a slot's buffers are not the
    // ones it lists (more slots).  A slot's buffers are its own for good -- select_kv moves pointers between the layers and the
    // parked slot, never between slots -- so a call is ONE launch that indexes the table.  A replaced table is parked in
    // kvc_retired until the model goes: an earlier launch may still read it and nothing here waits for the stream.
    DevPin<void *> kvc_tab;
    std::vector<void *> kvc_tab_host;          // what the device table holds
    std::vector<DevPin<void *>> kvc_retired;   // replaced tables
    DevBuf<float> kvs_rot;                     // context shift (ifa_model_kv_shift, ifa_kv_shift.hip): [head_dim / 2] (cos, sin) of the last call's rotation
    // Sampled decode (ifa_model_decode_sampled, ifa_engine_sampled.hip).  samp_blk: the call's parameters, generator state, state
    // slot and error word in device memory (+ pinned twin).  samp_graphs: the captured sampled step per
    // (KV slot << 10 | k << 1 | armed) -- what the tail bakes into its launches -- with the buffer addresses it names; the greedy
    // step's graphs are not among them.
    struct SampGraph { hipGraphExec_t exec = nullptr; const void *ptrs[8] = {}; };
    std::map<int, SampGraph> samp_graphs;
    DevPin<SampBlk> samp_blk;
    // Sampled draft step (ifa_model_decode_draft_sampled, ifa_engine_draft_sampled.hip): the call's parameters, state slot, draft
    // tokens, generator state and results in device memory (+ pinned twin).
    DevPin<DraftBlk> draft_blk;
    static constexpr int RING = 1024;
};


static inline bool is_q4(int dt) { return dt == Q4_B32T1A || dt == Q4_B32T1B; }

// formats the MO copy of the rows GEMM takes: 4-bit codes with value q * scale + base (the 64-weight ones only through MO)
static inline bool rows_mo_fmt(int dt) { return is_q4(dt) || dt == Q4_B64T1 || dt == Q3H_B64T1; }

static inline bool scale_on(float s) { return s < 0.9999f || s > 1.0001f; }     // the reference's test for "scale != 1"

// same tiled layout and arithmetic (the A/B variants differ only in how the quantizer picked base/scale)
static inline bool same_fmt(int a, int b) { return a == b || (is_q4(a) && is_q4(b)); }


static inline int num_cus() { return dec_num_cus(); }


// The fused GEMV of a weight tensor: int8-path formats stream their tiled copy (k_dec_gemv), everything else -- F16
// tensors, Q8_B32T1 / Q5_B32T1 / Q4_B16 / Q3_B32T1 / Q2_B32T1 -- the reference-layout bytes with fp16 activations
// (k_dec_gemv_h).  wbytes() hands out the matching pointer.
static inline bool fused_int8(int w_dtype) { return ax8_eligible(w_dtype); }

static inline const uint8_t *wbytes(const Tensor &t) { return (const uint8_t *)(fused_int8(t.dtype) ? t.tiled.get() : t.data.get()); }


extern "C" int ifa_add_layernorm(int kind, const void *a, const void *addend, size_t rows, size_t cols, const void *w, const void *b,
                                 float multi_base, float eps, void *sum_out, void *y, ifa_stream stream);

extern "C" int ifa_rope_qk_store(void *q, void *k, const void *v, int head_dim, int heads, int kv_heads, int tokens, int pos0, float theta,
                                 int order, float partial_rotary_factor, void *kcache_rows, void *vcache_rows, size_t cache_row_elems,
                                 ifa_stream stream);

extern "C" int ifa_activation_mul(int kind, const void *a, const void *b, size_t n, void *c, ifa_stream stream);

extern "C" int ifa_argmax_rows(const void *logits, size_t n, size_t row_stride, size_t rows, int *out_dev, const int *excluded_dev, ifa_stream stream);

extern "C" int ifa_gemm_rows_q4(const void *Wt_tiled, size_t rows, size_t cols, const void *x_f16, size_t tokens,
                                const void *bias_f16, void *y_f16, ifa_stream stream);

namespace ifa {     // ifa_moe.hip / ifa_gemm.hip / ifa_gemv.hip
int moe_build_lists(const int *sel, const void *wsel, int T, int top_k, int E, int tile_rows, int small_max, int *idx, void *wdev, int *epos,
                    MoeTile *tiles, MoeSingle *singles, MoeTile *smalls, int *counts, hipStream_t s);
int gemm_rows_q4_grouped_cap(size_t cols);
bool gemm_rows_use_mfma();
bool gemm_rows_mfma_ok(size_t rows, size_t cols, size_t tokens);
int gemm_rows_mfma_grouped(const MoeSmallGroup &grp, size_t rows, size_t cols, const void *X, void *Y, int max_groups, int max_rows, hipStream_t s);
int gemm_rows_mo_grouped(const MoeSmallGroup &grp, size_t rows, size_t cols, const void *X, void *Y, int max_groups, int glu, int act_kind, hipStream_t s);
int gemm_rows_q4_grouped(const MoeSmallGroup &grp, size_t rows, size_t cols, const void *X, void *Y, int max_groups, hipStream_t s);
int moe_gather(const void *src, const int *idx, const int *counts, int max_entries, int dim, void *dst, hipStream_t s);
int moe_combine(const void *y, const int *epos, const void *wsel, int T, int top_k, int dim, void *out, hipStream_t s, const void *residual = nullptr);
int gemm_q_grouped(int w_dtype, const MoeGroup &grp, size_t N, size_t K, const void *X, void *Y, int max_tiles, int tile_rows, hipStream_t s);
int gemv_ax8_grouped(int w_dtype, const MoeGroup &grp, size_t rows, size_t cols, const void *xq8_rows, void *y_rows, int max_singles,
                     hipStream_t s);
}


// ------------------------------------------------ dynamic batching: one new token for each of n queries
// (QueryStateTable + Infer_Std over several queries, src/transformer/inference_engine.cc:1054-1220): the linear layers
// run once over the n rows (weights streamed once: MFMA GEMM), RoPE / KV store / attention per row on the KV cache
// set of its query.
struct AttnRowH { const void *kc, *vc; int n_ctx, pad; };

extern "C" int ifa_attention_rows(const void *q, const void *rows_dev, int kv_dtype, int n_rows, int max_ctx, int heads, int kv_heads,
                                  int head_dim, float kq_scale, int alibi, int alibi_base_head, int alibi_total_heads, void *out,
                                  ifa_stream stream);

extern "C" int ifa_rope_rows(void *x, int head_dim, int heads, int tokens, const int *positions_dev, float theta, int order,
                             float partial_rotary_factor, ifa_stream stream);

namespace ifae {

// "raise the dynamic-LDS attribute when over 48 KiB, then launch"
template <class K, class... Args>
static int launch_lds(K kern, dim3 grid, dim3 block, size_t smem, hipStream_t s, Args... args)
{
    if (smem > 48 * 1024) IFA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    kern<<<grid, block, smem, s>>>(args...);
    IFA_LAUNCH_CHECK();
    return IFA_OK;
}

// f(head_dim constant, Q8-cache constant) over the pairs the attention kernels exist for: 32 / 64 / 96 / 128 with an F16 or a Q8 cache,
// 48 / 80 (no whole Q8 blocks) with an F16 cache only
template <class F>
static int attn_dispatch(int head_dim, bool q8, F &&f)
{
    using std::integral_constant;
    switch (head_dim) {
    case 32: return q8 ? f(integral_constant<int, 32>{}, std::true_type{}) : f(integral_constant<int, 32>{}, std::false_type{});
    case 64: return q8 ? f(integral_constant<int, 64>{}, std::true_type{}) : f(integral_constant<int, 64>{}, std::false_type{});
    case 96: return q8 ? f(integral_constant<int, 96>{}, std::true_type{}) : f(integral_constant<int, 96>{}, std::false_type{});
    case 128: return q8 ? f(integral_constant<int, 128>{}, std::true_type{}) : f(integral_constant<int, 128>{}, std::false_type{});
    case 48: if (!q8) return f(integral_constant<int, 48>{}, std::false_type{}); break;
    case 80: if (!q8) return f(integral_constant<int, 80>{}, std::false_type{}); break;
    }
    return ifa_fail(IFA_ERR_ARG, "fused attention: head_dim %d with %s cache", head_dim, q8 ? "a Q8" : "an F16");
}

// ---- ifa_engine.hip
void drop_graphs(ifa_model *m);
// One body of launches as an instantiated graph: synchronise, begin capture, run body, end capture, instantiate.  The hipGraph_t is
// destroyed on every failing path -- and on success too unless `keep` is given, whose old graph it then replaces.
template <class F>
static int capture_graph(ifa_model *m, const char *what, hipGraphExec_t *exec, hipGraph_t *keep, F &&body)
{
    hipStream_t s = m->stream;
    IFA_HIP_CHECK(hipStreamSynchronize(s));
    IFA_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t gph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &gph);
    if (rc || e != hipSuccess) {
        if (gph) (void)hipGraphDestroy(gph);
        return rc ? rc : ifa_fail(IFA_ERR_HIP, "hipStreamEndCapture (%s): %s", what, hipGetErrorString(e));
    }
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, gph, nullptr, nullptr, 0);
    if (ei != hipSuccess || !keep) (void)hipGraphDestroy(gph);
    if (ei != hipSuccess) return ifa_fail(IFA_ERR_HIP, "hipGraphInstantiate (%s): %s", what, hipGetErrorString(ei));
    if (keep) { if (*keep) (void)hipGraphDestroy(*keep); *keep = gph; }
    *exec = ex;
    return IFA_OK;
}
// what every entry point with a tail on the device refuses: a partitioned worker (its vocabulary is sharded), a pipeline stage
// without lm_head (needs_embd: or embeddings) and -- fused_only: the tail hangs on the fused, captured step -- options exact_order / perf_stat.
// device_tail_refusal: the reason or null, nothing recorded; device_tail_refusals: IFA_ERR_STATE with "who: reason; hint" (hint: what
// the caller can do instead)
const char *device_tail_refusal(const ifa_model *m, bool needs_embd, bool fused_only);
int device_tail_refusals(const ifa_model *m, const char *who, bool needs_embd, bool fused_only, const char *hint);
// perf_stat spans (ifa_engine.hip): no-ops unless the option is on.  PerfSpan brackets a phase on the model's stream.
int perf_begin(ifa_model *m, int key);
void perf_end(ifa_model *m, int idx);
int perf_collect(ifa_model *m);
struct PerfSpan {
    ifa_model *m; int idx;
    PerfSpan(ifa_model *mm, int key, bool on = true) : m(mm), idx(on ? perf_begin(mm, key) : -1) {}
    ~PerfSpan() { done(); }
    void done() { if (idx >= 0) { perf_end(m, idx); idx = -1; } }
};
void *kv_ptr(ifa_model *m, size_t layer, int slot, bool is_v);
// ---- ifa_kv_copy.hip: the device table of every slot's K / V buffers lists what slots a and b have now (restaged on the model's stream if not)
int kv_copy_table(ifa_model *m, int a, int b);
int ensure_mo(ifa_model *m);
int ensure_mo_build(ifa_model *m);
int ensure_x32(ifa_model *m);
int ensure_q3hn(ifa_model *m);
int ensure_scratch(ifa_model *m, int T);
// ---- ifa_engine_decode.hip
bool fused_ok(const Tensor &t, bool long_rows);
int lmhead_grid(const DecLmHeadParams &P, int wgs_per_cu_opt);
int launch_lmhead(const DecLmHeadParams &P, int norm, int wgs_per_cu_opt, hipStream_t s, const DecStepTail *Z = nullptr);
bool has_post_norms(const ifa_model *m);
bool fused_supported(const ifa_model *m, std::string *why);
int sep_norm(ifa_model *m, const half_t *x, const Tensor &w, const Tensor &b, half_t *dst);
void attn_params(ifa_model *m, int l, DecAttnParams &A);      // (the batch-1 step's; batch_fused_layer overrides the per-row fields)
int decode_route_ready(ifa_model *m, int reach, bool own_launches = false);
void qkv_params(ifa_model *m, int l, const half_t *x, DecGemvParams &P);
int launch_qkv_attn(ifa_model *m, int l, const half_t *x, unsigned tag_add = 0);
int launch_qkv(ifa_model *m, int l, const half_t *x);
int launch_attn(ifa_model *m, int l);
int launch_wo(ifa_model *m, int l, const half_t *x, half_t *partial = nullptr);
void moe_params(ifa_model *m, Layer &L, DecGemvParams &P, int slot, int tab_off);
int launch_ffn13(ifa_model *m, int l, int moe_slot = -1, const half_t *x_layer = nullptr, int moe_nslots = 1);
int launch_w2(ifa_model *m, int l, half_t *xnext, half_t *partial = nullptr, int moe_slot = -1, bool moe_last = false,
                     const half_t *residual2 = nullptr, int moe_t1_slot = 0);
int launch_chain(ifa_model *m, int l, const half_t *x, half_t *xnext, unsigned tag_add = 0);
bool step_tail_ok(const ifa_model *m);
DecLmHeadParams lm_params(ifa_model *m, const half_t *x, half_t *logits_out);
int step_tail_ready(ifa_model *m);
int launch_lm_tail(ifa_model *m, const half_t *x);
int launch_gather(ifa_model *m);
int launch_lm(ifa_model *m, const half_t *x, half_t *logits_out = nullptr);
// a fused step ends in the greedy argmax (k_dec_lmhead_tail, or lm_head + k_dec_argmax_advance) unless its tail is TAIL_SAMPLED: then in
// the draw (sampled_tail_enqueue)
int enqueue_fused_step(ifa_model *m, const StepTail &t);
// (a TAIL_SAMPLED call comes from ifa_model_decode_sampled, which has checked that the fused graph route is open)
int decode_impl(ifa_model *m, int first_token, int start_pos, int n_steps, int *out_tokens_host, float *elapsed_ms, bool prepare_only,
                const StepTail &t, TailCursor &cur);
// ---- ifa_engine_sampled.hip
int sampled_prepare(ifa_model *m, const StepTail &t);
int sampled_tail_enqueue(ifa_model *m, const StepTail &t, const half_t *x);
int sampled_graph(ifa_model *m, const StepTail &t, hipGraphExec_t *exec_out);
void sampled_drop_graphs(ifa_model *m);
int sampled_begin(ifa_model *m, const SampledCall &sc);
int sampled_copy_back(ifa_model *m);
int sampled_finish(ifa_model *m, const SampledCall &sc);
// ---- ifa_engine_forward.hip
int gather_rows(ifa_model *m, const half_t *src, const int *idx_dev, int T, int dim, int n_src, half_t *dst, float scale);
int matmul(ifa_model *m, const half_t *A, int T, const Tensor &W, const Tensor &bias, half_t *C);
int norm_rows(ifa_model *m, const half_t *x, int T, const Tensor &w, const Tensor &b, half_t *y, float base = 0.0f);
int ffn_dense(ifa_model *m, const half_t *x, int T, const Tensor &w1, const Tensor &b1, const Tensor &w3, const Tensor &b3,
                     const Tensor &w2, const Tensor &b2, half_t *out, int perf_base = 0);
int layer_tail_ops(ifa_model *m, int l, int T, half_t *&x, const half_t *attn_in, bool &xn_ready);
int prompt_route_ready(ifa_model *m, int T, int prefix_len, bool entry, PromptRoute &R);
int forward_ops(ifa_model *m, const int *tokens_host, int T, int prefix_len, void *logits_out, int *next_token, const StepTail &t, TailCursor &cur,
                bool no_head = false, const PromptRoute *planned = nullptr);
// ifa_model_forward behind its argument checks: one pass, the two passes of a 34..48-token prompt, or exact_order's row-by-row steps
int forward_impl(ifa_model *m, const int *tokens_host, int n_tokens, int prefix_len, void *logits_out_dev, int *next_token_host,
                 const StepTail &t, TailCursor &cur);
// ifa_decode_draft_kv.hip: RoPE + cache rows of the n rows of a draft step (rows_l: the layer's AttnRowH[n]) in one launch
int draft_kv_store_launch(ifa_model *m, int n, const half_t *k, const half_t *v, int stride, const void *rows_l);
int batch_route_of_call(ifa_model *m, int n, BatchRoute &R);
// TAIL_FED (ifa_model_decode_batch_steps; fused + captured routes only): the call's first step uploads its tables in front of the replay,
// a later one replays on the tables as the device left them; both only enqueue.  draft: the rows share a slot (ifa_model_decode_draft)
int forward_batch(ifa_model *m, int n, const int *tokens_host, const int *pos_host, const int *slot_host, int *next_tokens,
                  void *logits_out, const StepTail &t, TailCursor &cur, bool draft = false);
// ifa_model_decode_batch behind its argument checks: one step, balanced chunks, or exact_order's rows one by one
int decode_batch_impl(ifa_model *m, int n, const int *tokens_host, const int *positions_host, const int *kv_slots_host, int *next_tokens_host,
                      void *logits_out_dev, const StepTail &t, TailCursor &cur);
// ---- ifa_engine_pool.hip
// What the step's tail enqueues behind `logits` ([n_rows][vocab], this step's rows) on the model's stream: called by every step at
// one place, in front of its synchronisation, never under capture.  TAIL_NONE / _SAMPLED / _FED: nothing.
int tail_enqueue(ifa_model *m, const StepTail &t, TailCursor &cur, const half_t *logits, int n_rows);
// "[logit processors ->] pool [-> log-sum-exp]" of the pooled rows [ja, jb) of block B (k entries a row).  idx: device row indices
// into `logits` for row ja on, null: rows [0, jb - ja).  slots: device state slots for row ja on -- the rows pass through
// ifa_logit_adjust_rows into la_adj rows [ja, jb) and are pooled from there -- null: raw.  The one place the pool launches.
int pool_rows_launch(ifa_model *m, const PoolBlock &B, int k, const half_t *logits, const int *idx, const int *slots, int ja, int jb);
// device / pinned staging for n_sel rows of k entries (grown on demand, outside any capture)
int pool_reserve(ifa_model *m, int n_sel, int k);
// la_adj for `rows` adjusted rows (at least 8; never shrinks; synchronises before it reallocates)
int la_adj_reserve(ifa_model *m, size_t rows, const char *who);
// checks and reservations of a call that pools n_sel rows with k entries; adj: what ifa_model_pool_adjust armed for it (emptied when
// no row is armed)
int pool_ready(ifa_model *m, int k, int n_sel, std::vector<int> &adj, const char *who);
// where the block's second half starts: row indices [cap / 2] | state slots of armed rows [cap / 2]
static inline size_t pool_idx_rows(const ifa_model *m) { return m->pool_idx.cap() / 2; }
// ifa_engine_draft_sampled.hip: TAIL_DRAFT_VERIFY on the n rows of `logits`, enqueue-only
int draft_sampled_enqueue(ifa_model *m, const StepTail &t, const half_t *logits, int n_rows);
// ---- ifa_engine_score.hip
static constexpr size_t LSE_PART_FLOATS = 256;      // rows * splits <= 128 pairs whatever the row count (ifa_logprob.hip, lse_splits)
int lse_part_reserve(ifa_model *m);
// TAIL_SCORE: the row log-sum-exp + target gather over `logits` ([n_rows][vocab], the next n_rows rows of the prompt); after the last
// row the copy of the 2 * n floats into pinned staging
int score_enqueue(ifa_model *m, const StepTail &t, TailCursor &cur, const half_t *logits, int n_rows);
// ---- ifa_engine_moe.hip
int launch_moe_router(ifa_model *m, int l);
// Mixture of experts (ProcessGpuLayer_Moe, inference_worker.cc:1924-2146): router GEMV -> softmax -> D2H ->
// host top-k (HostTensorOpr::BuildRowsForMoE, host_tensor_opr.cc:190-244: probabilities below 1e-5 are dropped,
// optional renormalisation) -> the selected experts' FFNs in ascending expert order, each row on the T=1
// path -> B[row] = hfma(out, weight, B[row]) (AddByRowIdx_Kernel).  Result in m->f.
// moe_plan: what the layer would run over T rows now (ifa_moe_plan.h; caller_norm: the caller leaves the FFN norm and the residual to the
// layer); moe_layer runs it.  pre_norm / residual / out: with the plan's fused rows router only (the rows before the norm, the residual
// Add in the combine launch, its result).
MoePlan moe_plan(const ifa_model *m, const Layer &L, int T, bool caller_norm);
int moe_layer(ifa_model *m, Layer &L, const MoePlan &P, const half_t *ff_n, int T, const half_t *pre_norm = nullptr, const half_t *residual = nullptr, half_t *out = nullptr);
int ensure_side_stream(ifa_model *m);
// ---- ifa_engine_exact.hip
bool exact_supported(const ifa_model *m, std::string *why);
int forward_exact(ifa_model *m, int token, int pos, void *logits_out, int *next_token, const StepTail &t, TailCursor &cur);
// ---- ifa_engine_tp.hip
int tp_argmax_scratch(ifa_model *m, size_t n_rows);
int tp_pick_rows(ifa_model *m, const ifa_tp_topology &t, const half_t *shard, size_t row_stride, int shard_rows, int n_rows);
bool tp_merging(const ifa_model *m);
int tp_merge_rows(ifa_model *m, half_t *buf, int T, const Tensor &bias);
int tp_ready(ifa_model *m);
int tp_flush_pending(ifa_model *m);
int tp_buffers(ifa_model *m);
int tp_step(ifa_model *m, const ifa_tp_topology &t, int token, int pos, bool want_token = true, void *logits_copy = nullptr);
int tp_check(ifa_model *m, const ifa_tp_topology *topo, const char *who);
int tp_oneshot_status(ifa_model *m, const ifa_tp_topology &t, const char *who);

} // namespace ifae
