// engine_config.cc -- the engine's .ini: InferenceEngine::LoadConfig and the settings checks Init shares with it.
#include <cstdlib>

#include "inferflow_amd.h"
#include "inference_engine.h"
#include "ifa_ini.h"

namespace inferflow_amd {

static bool LoadDeviceGroups(std::vector<std::vector<int>> &groups, const IniConfig &cfg, const std::string &section, const std::string &key)
{
    // "0;1" = two groups (by layer), "0&1" = one group of two (by tensor)  (inference_engine.cc:1738-1783)
    groups.clear();
    std::string str;
    cfg.GetItem(section, key, str);
    for (std::string tok : IniConfig::Split(str, ",;")) {
        tok = IniConfig::Trim(tok);
        if (tok.empty()) continue;
        std::vector<int> sub;
        for (std::string s : IniConfig::Split(tok, "&|")) { s = IniConfig::Trim(s); if (!s.empty()) sub.push_back(atoi(s.c_str())); }
        groups.push_back(sub);
    }
    for (size_t g = 1; g < groups.size(); g++)
        if (groups[g].size() != groups[0].size()) {
            EngineSetError("All device groups should have the same size: %zu vs. %zu", groups[0].size(), groups[g].size());
            return false;
        }
    return true;
}

static bool LoadModelSpec(ModelSpec &spec, const IniConfig &cfg, const std::string &section)
{
    if (!cfg.GetItem(section, "model_dir", spec.dir) || spec.dir.empty()) {
        EngineSetError("The directory of model \"%s\" should not be empty", spec.sid.c_str()); return false;
    }
    if (spec.dir.back() != '/' && spec.dir.back() != '\\') spec.dir += '/';
    if (!cfg.GetItem(section, "model_specification_file", spec.spec_file)) cfg.GetItem(section, "model_spec_file", spec.spec_file);
    if (spec.spec_file.empty()) { EngineSetError("The specification file of model \"%s\" should not be empty", spec.sid.c_str()); return false; }
    cfg.GetItem(section, "decoding_strategy", spec.decoding_strategy);
    cfg.GetItem(section, "decoder_input_template", spec.decoder_input_template);
    cfg.GetItem(section, "prompt_template", spec.decoder_input_template);
    std::string str;
    if (cfg.GetItem(section, "device_weight_data_type", str) && !str.empty()) {
        const int dt = ifa_dtype_from_name(IniConfig::Lower(str).c_str());
        if (dt < 0) { EngineSetError("Invalid device_weight_data_type for model %s", spec.sid.c_str()); return false; }
        spec.device_weight_data_type = dt;
    }
    {   // device_weight_data_type.<tensor>: element size >= 2 -> F16 (inference_engine.cc:1685-1687)
        static const struct { const char *name; int tid; } kTensors[] = {{"attn_wq", IFA_T_WQ}, {"attn_wk", IFA_T_WK}, {"attn_wv", IFA_T_WV},
            {"attn_wo", IFA_T_WO}, {"ffn_w1", IFA_T_W1}, {"ffn_w2", IFA_T_W2}, {"ffn_w3", IFA_T_W3}};
        for (const auto &kt : kTensors) {
            std::string v;
            if (!cfg.GetItem(section, std::string("device_weight_data_type.") + kt.name, v) || v.empty()) continue;
            const int dt = ifa_dtype_from_name(IniConfig::Lower(v).c_str());
            if (dt < 0) { EngineSetError("Invalid device_weight_data_type.%s for model %s", kt.name, spec.sid.c_str()); return false; }
            spec.device_weight_data_types[kt.tid] = (dt == IFA_F32 || dt == IFA_F16) ? IFA_F16 : dt;
        }
    }
    str.clear();
    if (cfg.GetItem(section, "device_kv_cache_data_type", str) && !str.empty()) {
        const int dt = ifa_dtype_from_name(IniConfig::Lower(str).c_str());
        if (dt < 0) { EngineSetError("Invalid device_kv_cache_data_type for model %s", spec.sid.c_str()); return false; }
        // element size >= 2 -> F16, anything smaller -> Q8_B32T2   (inference_engine.cc:1701-1703)
        spec.device_kv_cache_data_type = (dt == IFA_F32 || dt == IFA_F16) ? IFA_F16 : IFA_Q8_B32T2;
    }
    cfg.GetItem(section, "tensor_quant_threshold", spec.tensor_quant_threshold);
    if (!LoadDeviceGroups(spec.device_groups, cfg, section, "devices")) return false;
    cfg.GetItem(section, "max_context_len", spec.max_context_len);
    const bool is_abs = !spec.spec_file.empty() && spec.spec_file[0] == '/';
    return LoadModelSpecJson(spec, is_abs ? spec.spec_file : spec.dir + spec.spec_file);
}

bool LookupConfigOk(const InferenceConfig &c)
{
    if (c.lookup_draft_len < 1 || c.lookup_draft_len > 7) { EngineSetError("lookup_draft_len must be 1..7 (got %d)", c.lookup_draft_len); return false; }
    if (c.lookup_ngram_min < 1 || c.lookup_ngram_max < c.lookup_ngram_min) {
        EngineSetError("lookup_ngram_min must be at least 1 and lookup_ngram_max no smaller (got %d, %d)", c.lookup_ngram_min, c.lookup_ngram_max);
        return false;
    }
    return true;
}

bool InferenceEngine::LoadConfig(InferenceConfig &config, const std::string &config_path,
                                 const std::string &section, const std::string &data_root_dir)
{
    IniConfig cfg; std::string err;
    if (!cfg.Load(config_path, &err)) { EngineSetError("Failed to load the configuration file: %s", err.c_str()); return false; }
    std::string root = data_root_dir;
    if (root.empty()) { IniConfig probe; probe.Load(config_path); probe.GetItem("app_env.base", "data_root_dir", root); }
    if (!root.empty()) cfg.AddMacro("data_root_dir", root);
    config.data_dir = root;
    std::string global_model_dir;
    cfg.GetItem("main", "global_model_dir", global_model_dir);
    cfg.AddMacro("global_model_dir", global_model_dir);
    if (!cfg.HasSection(section)) { EngineSetError("Section [%s] is missing in %s", section.c_str(), config_path.c_str()); return false; }
    if (!LoadDeviceGroups(config.device_groups, cfg, section, "devices")) return false;
    if (config.device_groups.empty()) config.device_groups.push_back({0});
    int cpu_layers = 0;
    if (cfg.GetItem(section, "cpu_layer_count", cpu_layers)) config.decoder_cpu_layer_count = cpu_layers;
    cfg.GetItem(section, "encoder_cpu_layer_count", config.encoder_cpu_layer_count);
    cfg.GetItem(section, "decoder_cpu_layer_count", config.decoder_cpu_layer_count);
    std::string models;
    if (!cfg.GetItem(section, "models", models) || IniConfig::Trim(models).empty()) {
        EngineSetError("Item \"models\" is missing in section [%s]", section.c_str()); return false;
    }
    config.models.clear();
    for (std::string name : IniConfig::Split(models, ",;")) {
        name = IniConfig::Trim(name);
        if (name.empty()) continue;
        ModelSpec spec; spec.sid = name;
        cfg.AddMacro("model_name", name);
        if (!LoadModelSpec(spec, cfg, "model." + name)) return false;
        if (spec.device_groups.empty()) spec.device_groups = config.device_groups;
        config.models.push_back(spec);
    }
    cfg.GetItem(section, "max_concurrent_queries", config.max_concurrent_queries);
    cfg.GetItem(section, "cpu_threads", config.cpu_threads);
    cfg.GetItem(section, "return_output_tensors", config.return_output_tensors);
    cfg.GetItem(section, "dynamic_batching_min_queries", config.dynamic_batching_min_queries);
    cfg.GetItem(section, "force_partition_path", config.force_partition_path);
    cfg.GetItem(section, "device_sampling_pool", config.device_sampling_pool);
    cfg.GetItem(section, "device_sampler", config.device_sampler);
    cfg.GetItem(section, "prefix_cache", config.prefix_cache);
    cfg.GetItem(section, "prefix_cache_min_tokens", config.prefix_cache_min_tokens);
    if (config.prefix_cache_min_tokens < 1) { EngineSetError("prefix_cache_min_tokens must be at least 1 (got %d)", config.prefix_cache_min_tokens); return false; }
    cfg.GetItem(section, "context_shift", config.context_shift);
    cfg.GetItem(section, "context_shift_keep", config.context_shift_keep);
    if (config.context_shift_keep < 0) { EngineSetError("context_shift_keep must be at least 0 (got %d)", config.context_shift_keep); return false; }
    cfg.GetItem(section, "batch_generate_round_steps", config.batch_generate_round_steps);
    if (config.batch_generate_round_steps < 1 || config.batch_generate_round_steps > 256) {
        EngineSetError("batch_generate_round_steps must be 1..256 (got %d)", config.batch_generate_round_steps); return false;
    }
    cfg.GetItem(section, "lookup_draft_len", config.lookup_draft_len);
    cfg.GetItem(section, "lookup_ngram_max", config.lookup_ngram_max);
    cfg.GetItem(section, "lookup_ngram_min", config.lookup_ngram_min);
    if (!LookupConfigOk(config)) return false;
    cfg.GetItem(section, "lookup_sampled", config.lookup_sampled);
    cfg.GetItem(section, "is_study_mode", config.debug.is_study_mode);
    cfg.GetItem(section, "show_tensors", config.debug.show_tensors);
    return true;
}

} // namespace inferflow_amd
