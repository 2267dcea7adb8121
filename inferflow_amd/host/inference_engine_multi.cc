// inference_engine_multi.cc -- InferenceEngine over a multi-GPU partition (devices = 0&1 | 0;1 | 0&1;2&3): the rank threads, the
// steps every rank takes at once and the assembly of the last group's vocabulary shards.  Everything that looks inside MultiGpu is here.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "inferflow_amd.h"
#include "inference_engine.h"

namespace inferflow_amd {

// ---------------------------------------------------------------------------------------------- multi-GPU partitions
// One worker (ifa_model) and one persistent host thread per GPU.  The reference creates and joins a thread per GPU inside
// every Infer() (inference_engine.cc:1203-1206, 1261-1283) and lets the workers rendezvous through GpuInfGlobalData's
// mutex; here the threads live as long as the engine and every exchange is a collective of the C ABI enqueued on the
// worker's stream (csrc/ifa_comm.hip), so a thread only ever blocks at the end of its step.
struct InferenceEngine::MultiGpu {
    std::vector<WorkerPlan> plans;
    std::vector<ifa_comm *> world, tp;          // per rank (world: only with several device groups; tp: only with groups of > 1)
    std::vector<ifa_tp_topology> topo;
    std::vector<void *> shard_dev;              // per rank: logits shard buffer [rows][V / P] (last group only)
    size_t shard_rows = 0;
    int G = 1, P = 1;
    bool force_collectives = false;
    // thread pool
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::function<int(int)> job;
    uint64_t generation = 0;
    int pending = 0;
    bool stop = false;
    int first_failed = -1;
    bool broken = false;      // a rank failed inside a step: the communicators were aborted, the engine cannot continue
    std::vector<std::string> errors;

    // A rank that fails before or between the collectives of a step leaves its peers blocked in theirs (RCCL, or the
    // loopback group's rendezvous) and Run() would never return.  The failing rank's thread aborts every communicator of
    // the job: the peers come back with an error, Run() reports the FIRST failure.
    void AbortGroups()
    {
        for (ifa_comm *c : tp) if (c) ifa_comm_abort(c);
        for (ifa_comm *c : world) if (c) ifa_comm_abort(c);
    }

    void Start()
    {
        const int n = (int)plans.size();
        errors.assign((size_t)n, std::string());
        for (int r = 0; r < n; r++)
            threads.emplace_back([this, r]() {
                uint64_t seen = 0;
                for (;;) {
                    std::function<int(int)> fn;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_job.wait(lk, [&] { return stop || generation != seen; });
                        if (stop) return;
                        seen = generation; fn = job;
                    }
                    const int rc = fn(r);
                    bool first_failure = false;
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        errors[(size_t)r] = rc == 0 ? std::string() : std::string(ifa_last_error());   // (thread-local message)
                        if (rc != 0 && errors[(size_t)r].empty()) errors[(size_t)r] = "error " + std::to_string(rc);
                        if (rc != 0 && !broken) { broken = true; first_failure = true; first_failed = r; }
                    }
                    if (first_failure && plans.size() > 1) AbortGroups();
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_all();
                    }
                }
            });
    }
    // fn(rank) on every rank's thread at once; false + message if any failed
    bool Run(const std::function<int(int)> &fn, const char *what)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (broken) { EngineSetError("%s: the engine's device group was aborted after an earlier failure; create a new engine", what); return false; }
            job = fn; pending = (int)plans.size(); generation++;
        }
        cv_job.notify_all();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
        if (first_failed < 0) return true;      // (no rank fails without first_failed being set)
        const size_t r = (size_t)first_failed;  // the rank whose failure started it (the others only report the abort)
        EngineSetError("%s failed on rank %zu (device %d): %s", what, r, plans[r].device, errors[r].c_str());
        return false;
    }
    // One step on every rank: step(rank, lg) enqueues it, lg = where the rank writes its shard [rows][V / P] of the logits (null: none
    // wanted, or a rank outside the last group, which has none).  want_logits: `logits` receives [rows][V] assembled from the shards.
    bool Step(size_t rows, size_t V, bool want_logits, const char *what, const std::function<int(int, void *)> &step, std::vector<uint16_t> &logits)
    {
        const size_t shard = V / (size_t)P, last0 = (size_t)(G - 1) * (size_t)P;
        if (want_logits && rows > shard_rows) {
            shard_rows = 0;
            for (size_t i = last0; i < plans.size(); i++) {
                ifa_set_device(plans[i].device);
                if (shard_dev[i]) { ifa_free(shard_dev[i]); shard_dev[i] = nullptr; }
                if (ifa_malloc(&shard_dev[i], rows * shard * 2) != IFA_OK) { EngineSetError("logits buffer: %s", ifa_last_error()); return false; }
            }
            shard_rows = rows;
        }
        std::vector<std::vector<uint16_t>> host(plans.size());
        const bool ok = Run([&](int i) -> int {
            void *lg = want_logits ? shard_dev[(size_t)i] : nullptr;
            const int rc = step(i, lg);
            if (rc || !lg) return rc;
            host[(size_t)i].resize(rows * shard);
            return CopyToHostSync(plans[(size_t)i].model, host[(size_t)i].data(), lg, rows * shard * 2);
        }, what);
        if (!ok || !want_logits) return ok;
        logits.resize(rows * V);
        for (size_t r = 0; r < (size_t)P; r++)
            for (size_t row = 0; row < rows; row++) memcpy(&logits[row * V + r * shard], &host[last0 + r][row * shard], shard * 2);
        return true;
    }
    ~MultiGpu()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_job.notify_all();
        for (std::thread &t : threads) if (t.joinable()) t.join();
        for (size_t r = 0; r < plans.size(); r++) {
            if (r < shard_dev.size() && shard_dev[r]) { ifa_set_device(plans[r].device); ifa_free(shard_dev[r]); }
            if (plans[r].model) ifa_model_destroy(plans[r].model);
        }
        for (ifa_comm *c : tp) if (c) ifa_comm_destroy(c);
        for (ifa_comm *c : world) if (c) ifa_comm_destroy(c);
    }
};

// devices = G groups of P: workers in the reference's order (rank = group * P + position), layer ranges by
// SplitGpuLayers, BY_TENSOR slices inside a group (model_loader.cc), one communicator per group + one for the job
bool InferenceEngine::InitMulti(const std::vector<std::vector<int>> &groups)
{
    const int G = (int)groups.size(), P = (int)groups[0].size();
    if (P < 1) { EngineSetError("empty device group"); return false; }
    multi_ = new MultiGpu();
    MultiGpu &M = *multi_;
    M.G = G; M.P = P; M.force_collectives = config_.force_partition_path;
    std::vector<int> all_devices;
    for (int g = 0; g < G; g++)
        for (int r = 0; r < P; r++) {
            WorkerPlan w;
            w.device = groups[(size_t)g][(size_t)r]; w.stage = g; w.n_stages = G; w.tp_rank = r; w.tp_size = P;
            M.plans.push_back(w);
            all_devices.push_back(w.device);
        }
    // a device named more than once: only as "every rank on ONE device" (loopback groups of the C ABI: the multi-rank
    // paths on a 1-GPU box, tests); anything else is a configuration mistake
    bool dup = false, all_same = true;
    for (size_t i = 0; i < all_devices.size(); i++) {
        all_same = all_same && all_devices[i] == all_devices[0];
        for (size_t j = i + 1; j < all_devices.size(); j++) dup = dup || all_devices[i] == all_devices[j];
    }
    if (dup && !all_same) { EngineSetError("a device appears twice in `devices`"); return false; }
    if (!BuildWorkers(M.plans, spec_)) return false;
    const int R = G * P;
    M.world.assign((size_t)R, nullptr); M.tp.assign((size_t)R, nullptr);
    if (G > 1 && ifa_comm_init_all(all_devices.data(), R, M.world.data()) != IFA_OK) { EngineSetError("job communicator: %s", ifa_last_error()); return false; }
    if (P > 1 || M.force_collectives)
        for (int g = 0; g < G; g++)
            if (ifa_comm_init_all(groups[(size_t)g].data(), P, M.tp.data() + (size_t)g * P) != IFA_OK) { EngineSetError("group communicator: %s", ifa_last_error()); return false; }
    const int V = spec_.hyper_params.vocab_size;
    M.topo.resize((size_t)R);
    for (int i = 0; i < R; i++) {
        ifa_tp_topology &t = M.topo[(size_t)i];
        memset(&t, 0, sizeof(t));
        const int g = i / P, r = i % P;
        t.tp = M.tp[(size_t)i]; t.world = M.world[(size_t)i];
        t.stage = g; t.n_stages = G;
        t.prev_rank = g > 0 ? i - P : -1; t.next_rank = g + 1 < G ? i + P : -1;
        t.token_src = (G - 1) * P;                  // first rank of the last group announces the token
        t.vocab_offset = r * (V / P);
        t.force_collectives = M.force_collectives ? 1 : 0;
    }
    M.shard_dev.assign((size_t)R, nullptr);
    M.Start();
    model_ = M.plans[0].model;      // (handle for model_info-style queries; steps go through the rank threads)
    return true;
}

// one step of one query on every rank: n_new tokens from q.processed on; `next` = the greedy next token.  want_tensor:
// item.output_tensor receives the [n_new][vocab] logits assembled from the last group's vocabulary shards.
bool InferenceEngine::MultiStep(Query &q, int n_new, bool want_tensor, QueryInferenceResult &item, int &next)
{
    MultiGpu &M = *multi_;
    const int R = (int)M.plans.size(), V = spec_.hyper_params.vocab_size;
    std::vector<int> nexts((size_t)R, -1);
    const int *toks = q.tokens.data() + q.processed;
    const int start = q.processed, slot = q.kv_slot;
    if (!M.Step((size_t)n_new, (size_t)V, want_tensor, n_new == 1 ? "decode step" : "prompt step", [&](int i, void *lg) -> int {
            ifa_model *mm = M.plans[(size_t)i].model;
            const int rc = ifa_model_select_kv(mm, slot);
            if (rc) return rc;
            if (n_new == 1 && !lg) return ifa_model_tp_decode(mm, &M.topo[(size_t)i], toks[0], start, 1, &nexts[(size_t)i], nullptr);
            return ifa_model_tp_prefill(mm, &M.topo[(size_t)i], toks, n_new, start, lg, &nexts[(size_t)i]);
        }, item.output_tensor)) return false;
    next = nexts[(size_t)(R - 1)];
    for (int i = 0; i < R; i++)
        if (nexts[(size_t)i] != next) { EngineSetError("ranks disagree on the next token (%d vs %d)", nexts[(size_t)i], next); return false; }
    if (want_tensor) { item.output_rows = n_new; item.output_cols = V; }
    return true;
}

// One batched decode step of n queries over the (single) tensor-parallel device group: every rank's thread calls
// ifa_model_tp_decode_batch with the same rows; `all` (if wanted) receives the [n][vocab] logits assembled from the ranks'
// vocabulary shards.
bool InferenceEngine::MultiBatchStep(const std::vector<int> &toks, const std::vector<int> &pos, const std::vector<int> &slots,
                                     std::vector<int> &next, bool want_tensor, std::vector<uint16_t> &all)
{
    MultiGpu &M = *multi_;
    const int R = (int)M.plans.size(), n = (int)toks.size();
    std::vector<std::vector<int>> nexts((size_t)R, std::vector<int>((size_t)n, -1));
    if (!M.Step((size_t)n, (size_t)spec_.hyper_params.vocab_size, want_tensor, "batched decode step", [&](int i, void *lg) -> int {
            return ifa_model_tp_decode_batch(M.plans[(size_t)i].model, &M.topo[(size_t)i], n, toks.data(), pos.data(), slots.data(), nexts[(size_t)i].data(), lg);
        }, all)) return false;
    next = nexts[(size_t)(R - 1)];
    for (int i = 0; i < R; i++)
        if (nexts[(size_t)i] != next) { EngineSetError("ranks disagree on the next tokens of a batched step"); return false; }
    return true;
}

// Generate's decode call on every rank: k greedy steps from the query's last token, fed back on the devices; the last rank's tokens
// and the slowest rank's time
bool InferenceEngine::MultiDecode(const Query &q, int k, int *out, float *gpu_ms)
{
    MultiGpu &M = *multi_;
    const int R = (int)M.plans.size();
    std::vector<std::vector<int>> outs((size_t)R, std::vector<int>((size_t)k));
    std::vector<float> ms((size_t)R, 0.0f);
    const int first = q.tokens.back(), start = q.processed, slot = q.kv_slot;
    if (!M.Run([&](int i) -> int {
            ifa_model *mm = M.plans[(size_t)i].model;
            int rc = ifa_model_select_kv(mm, slot);
            return rc ? rc : ifa_model_tp_decode(mm, &M.topo[(size_t)i], first, start, k, outs[(size_t)i].data(), &ms[(size_t)i]);
        }, "decode")) return false;
    std::copy(outs[(size_t)(R - 1)].begin(), outs[(size_t)(R - 1)].end(), out);
    *gpu_ms = *std::max_element(ms.begin(), ms.end());
    return true;
}

// ---- what the rest of the engine asks of the partition
void InferenceEngine::FreeMulti() { delete multi_; multi_ = nullptr; }
int InferenceEngine::PartitionRanks() const { return multi_ ? (int)multi_->plans.size() : 1; }
int InferenceEngine::LayerGroups() const { return multi_ ? multi_->G : 1; }

std::vector<ifa_model *> InferenceEngine::Workers() const
{
    std::vector<ifa_model *> all;
    if (multi_) for (const WorkerPlan &w : multi_->plans) all.push_back(w.model); else all.push_back(model_);
    return all;
}

ifa_model *InferenceEngine::worker(int rank)
{
    if (!multi_) return rank == 0 ? model_ : nullptr;
    return rank >= 0 && rank < (int)multi_->plans.size() ? multi_->plans[(size_t)rank].model : nullptr;
}

bool InferenceEngine::WorkerPlanOf(int rank, int out6[6]) const
{
    if (rank < 0 || rank >= PartitionRanks()) return false;
    WorkerPlan w;                   // (a single device: one stage, one rank, every layer)
    w.layer1 = spec_.hyper_params.decoder_layers;
    if (multi_) w = multi_->plans[(size_t)rank];
    out6[0] = w.stage; out6[1] = w.n_stages; out6[2] = w.tp_rank; out6[3] = w.tp_size; out6[4] = w.layer0; out6[5] = w.layer1;
    return true;
}

} // namespace inferflow_amd
