"""Python view of the C++ InferenceEngine facade (inferflow_amd/host/inference_engine.h) through
include/inferflow_engine.h -- the reference's serving loop, same names and return conventions:

    eng = InferenceEngine.from_ini("llm_inference.ini", "transformer_engine")
    qid = eng.add_query(tokens)              # > 0 id, 0 busy, < 0 error
    while ...:
        for query_id, next_token in eng.infer():
            eng.commit({query_id: (next_token, False)})
    eng.remove_query(qid)
"""
import ctypes as C

import numpy as np

from . import _capi


class EngineError(RuntimeError):
    pass


class InferenceEngine:
    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _err():
        return _capi.lib().ifa_engine_last_error().decode(errors="replace")

    @classmethod
    def from_ini(cls, ini_path, section="transformer_engine", data_root_dir=""):
        h = _capi.lib().ifa_engine_create(str(ini_path).encode(), section.encode(), data_root_dir.encode())
        if not h:
            raise EngineError("LoadConfig/Init failed: " + cls._err())
        return cls(h)

    def close(self):
        if self._h:
            _capi.lib().ifa_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_query(self, tokens, strategy=None, seed=0, temperature=1.0, logprobs=-1, repetition_penalty=1.0, presence_penalty=0.0,
                  frequency_penalty=0.0, logit_bias=None, context_shift=None, context_keep=None):
        """strategy: None (the model's default) or a name / SamplingStrategyId ("sample.top_p", "greedy", 1 ...).
        logprobs: -1 off; 0: the chosen token's log-probability; 1..20: also the n most probable tokens (last_logprobs).
        repetition_penalty (HF rule, prompt + generated ids), presence_penalty / frequency_penalty (OpenAI rule, generated ids),
        logit_bias ({token id: value}, -inf bans the id): logit processors applied on the device in front of the candidate pool
        (include/inferflow_engine.h, ifa_engine_add_query_opt); a query with any of them takes the device pool route.
        context_shift: None (the engine's `context_shift` key), False, True -- the query runs past max_context_len by dropping old
        cache rows; context_keep: None (the engine's `context_shift_keep`) or the rows kept in front of the dropped block."""
        arr = (C.c_int * len(tokens))(*[int(t) for t in tokens])
        if repetition_penalty != 1.0 or presence_penalty != 0.0 or frequency_penalty != 0.0 or logit_bias or context_shift is not None or context_keep is not None:
            sid = 0 if strategy is None else (strategy if isinstance(strategy, int) else self.strategy_id(strategy))
            bias = sorted((logit_bias or {}).items())
            ids = (C.c_int * max(1, len(bias)))(*[int(k) for k, _ in bias])
            vals = (C.c_float * max(1, len(bias)))(*[float(v) for _, v in bias])
            opt = _capi.QueryOptionsShift(C.sizeof(_capi.QueryOptionsShift), int(sid), int(seed), float(temperature), int(logprobs), float(repetition_penalty),
                                          float(presence_penalty), float(frequency_penalty), len(bias), ids, vals,
                                          -1 if context_shift is None else int(bool(context_shift)), -1 if context_keep is None else int(context_keep))
            return _capi.lib().ifa_engine_add_query_opt(self._h, arr, len(tokens), C.byref(opt))
        if logprobs != -1:
            sid = 0 if strategy is None else (strategy if isinstance(strategy, int) else self.strategy_id(strategy))
            return _capi.lib().ifa_engine_add_query_lp(self._h, arr, len(tokens), int(sid), int(seed), float(temperature), int(logprobs))
        if strategy is None and seed == 0 and temperature == 1.0:
            return _capi.lib().ifa_engine_add_query(self._h, arr, len(tokens))
        sid = 0 if strategy is None else (strategy if isinstance(strategy, int) else self.strategy_id(strategy))
        return _capi.lib().ifa_engine_add_query_ex(self._h, arr, len(tokens), int(sid), int(seed), float(temperature))

    def strategy_id(self, name=""):
        return _capi.lib().ifa_engine_strategy_id(self._h, (name or "").encode())

    def query_count(self):
        return _capi.lib().ifa_engine_query_count(self._h)

    def remove_query(self, query_id):
        return bool(_capi.lib().ifa_engine_remove_query(self._h, query_id))

    def infer(self, capacity=64):
        """One Infer(): [(query_id, greedy next token)] for the queries that advanced."""
        ids = (C.c_int * capacity)()
        toks = (C.c_int * capacity)()
        n = _capi.lib().ifa_engine_infer(self._h, ids, toks, capacity)
        if n < 0:
            raise EngineError("Infer failed: " + self._err())
        return [(ids[i], toks[i]) for i in range(min(n, capacity))]

    def commit(self, query_map):
        """query_map: {query_id: token} or {query_id: (token, is_end)}"""
        n = len(query_map)
        ids = (C.c_int * n)(); toks = (C.c_int * n)(); ends = (C.c_int * n)()
        for i, (q, v) in enumerate(query_map.items()):
            tok, end = v if isinstance(v, tuple) else (v, False)
            ids[i], toks[i], ends[i] = q, int(tok), int(bool(end))
        return bool(_capi.lib().ifa_engine_commit(self._h, ids, toks, ends, n))

    def perf_stat(self):
        """{key: ms} of the last infer(): key 0 end to end; in study mode the reference's per-phase keys (include/inferflow_engine.h)"""
        keys = (C.c_uint * 256)(); ms = (C.c_float * 256)()
        n = _capi.lib().ifa_engine_perf_stat(self._h, keys, ms, 256)
        if n < 0:
            raise EngineError(self._err())
        return {int(keys[i]): float(ms[i]) for i in range(min(n, 256))}

    def last_logits(self, query_id):
        rows, cols = C.c_int(0), C.c_int(0)
        if not _capi.lib().ifa_engine_last_logits(self._h, query_id, None, 0, C.byref(rows), C.byref(cols)):
            raise EngineError(self._err())
        out = np.zeros((rows.value, cols.value), np.float16)
        if out.size:
            _capi.lib().ifa_engine_last_logits(self._h, query_id, out.ctypes.data_as(C.c_void_p), out.size, C.byref(rows), C.byref(cols))
        return out

    def last_logprobs(self, query_id, cap=32):
        """(log p of the token the query's last step chose, [(token id, log p)] of its most probable tokens, best first)"""
        chosen, n = C.c_float(0), C.c_int(0)
        ids = (C.c_int * cap)(); lps = (C.c_float * cap)()
        if not _capi.lib().ifa_engine_last_logprobs(self._h, int(query_id), C.byref(chosen), ids, lps, cap, C.byref(n)):
            raise EngineError(self._err())
        return chosen.value, [(ids[i], lps[i]) for i in range(min(n.value, cap))]

    def score(self, tokens):
        """float32 [len(tokens) - 1]: log p(tokens[i + 1] | tokens[:i + 1]), reduced on the device (InferenceEngine::ScoreTokens)"""
        arr = (C.c_int * len(tokens))(*[int(t) for t in tokens])
        out = np.zeros(max(len(tokens) - 1, 1), np.float32)
        if not _capi.lib().ifa_engine_score(self._h, arr, len(tokens), out.ctypes.data_as(C.POINTER(C.c_float))):
            raise EngineError("score failed: " + self._err())
        return out[:len(tokens) - 1]

    def generate(self, query_id, n_steps):
        out = (C.c_int * max(1, n_steps))()
        ms = C.c_float(0)
        n = _capi.lib().ifa_engine_generate(self._h, query_id, n_steps, out, C.byref(ms))
        if n < 0:
            raise EngineError("Generate failed: " + self._err())
        return [out[i] for i in range(n)], ms.value

    def generate_batch(self, items):
        """Generate for a set of queries (InferenceEngine::GenerateBatch): items = [(query_id, max_new_tokens) or (query_id,
        max_new_tokens, stop_token_ids)].  The live queries run rounds of device-fed batched steps -- one worker call and one
        synchronisation per round of at most `batch_generate_round_steps` steps -- and receive the tokens of the infer / commit loop;
        a query ends early at one of its (at most 8) stop ids.  Returns ({query_id: tokens}, {query_id: stopped}, {rounds,
        batched_steps, single_steps, gpu_ms})."""
        items = [(int(it[0]), int(it[1]), [int(t) for t in (it[2] if len(it) > 2 and it[2] is not None else ())]) for it in items]
        n = len(items)
        ia = lambda v: (C.c_int * max(1, len(v)))(*v)
        stop_off, out_off = [0], [0]
        for _, max_new, stops in items:
            stop_off.append(stop_off[-1] + len(stops))
            out_off.append(out_off[-1] + max(0, max_new))
        out = (C.c_int * max(1, out_off[-1]))()
        counts, stopped, st = (C.c_int * max(1, n))(), (C.c_int * max(1, n))(), (C.c_float * 4)()
        rc = _capi.lib().ifa_engine_generate_batch(self._h, n, ia([it[0] for it in items]), ia([it[1] for it in items]),
                                                   ia([t for it in items for t in it[2]]), ia(stop_off), out, ia(out_off), counts, stopped, st)
        if rc != 0:
            raise EngineError("GenerateBatch failed: " + self._err())
        toks = {items[i][0]: [out[out_off[i] + t] for t in range(counts[i])] for i in range(n)}
        stats = {"rounds": int(st[0]), "batched_steps": int(st[1]), "single_steps": int(st[2]), "gpu_ms": float(st[3])}
        return toks, {items[i][0]: bool(stopped[i]) for i in range(n)}, stats

    def generate_lookup(self, query_id, max_new_tokens, prediction=None):
        """Lookup decoding (InferenceEngine::GenerateLookup): up to max_new_tokens greedy tokens, draft tokens taken from
        `prediction` (token ids the output is expected to repeat; None: none) and from the query's own tokens, verified in one
        batched step per draft.  With `lookup_sampled = true` in the .ini also seeded sampled and processed queries: a draft is
        accepted where it equals the token drawn on the device.  Returns (tokens, {steps, draft_steps, drafted, accepted, gpu_ms})."""
        out = (C.c_int * max(1, max_new_tokens))()
        st = (C.c_float * 5)()
        pred = list(prediction) if prediction is not None else []
        arr = (C.c_int * len(pred))(*[int(t) for t in pred]) if pred else None
        n = _capi.lib().ifa_engine_generate_lookup(self._h, int(query_id), int(max_new_tokens), arr, len(pred), out, st)
        if n < 0:
            raise EngineError("GenerateLookup failed: " + self._err())
        stats = {"steps": int(st[0]), "draft_steps": int(st[1]), "drafted": int(st[2]), "accepted": int(st[3]), "gpu_ms": float(st[4])}
        return [out[i] for i in range(n)], stats

    def perplexity(self, tokens, max_length=512, stride=512, device_scoring=False):
        """(PPL, error estimate, scored tokens) of a token-id stream -- the reference's perplexity tool.  device_scoring: every
        window is scored on the device (an engine with return_output_tensors = false; the default needs it true)."""
        arr = (C.c_int * len(tokens))(*[int(t) for t in tokens])
        ppl, err, cnt = C.c_double(0), C.c_double(0), C.c_longlong(0)
        fn = _capi.lib().ifa_engine_perplexity_device if device_scoring else _capi.lib().ifa_engine_perplexity
        if not fn(self._h, arr, len(tokens), max_length, stride, C.byref(ppl), C.byref(err), C.byref(cnt)):
            raise EngineError("perplexity failed: " + self._err())
        return ppl.value, err.value, cnt.value

    def model_info(self, key):
        return _capi.lib().ifa_engine_model_info(self._h, key.encode())

    def query_cached_tokens(self, query_id):
        """Leading prompt tokens whose K/V rows add_query found in a slot (prefix_cache = true in the .ini); -1: unknown id"""
        return _capi.lib().ifa_engine_query_cached_tokens(self._h, int(query_id))

    def shift_query(self, query_id, keep, discard):
        """Context shift with the caller's numbers: tokens [keep, keep + discard) of the query and their cache rows are dropped, the
        rows behind them move down (InferenceEngine::ShiftQuery)"""
        if not _capi.lib().ifa_engine_shift_query(self._h, int(query_id), int(keep), int(discard)):
            raise EngineError("ShiftQuery failed: " + self._err())

    def query_shifted_tokens(self, query_id):
        """Tokens the query's context shifts have dropped so far; -1: unknown id"""
        return _capi.lib().ifa_engine_query_shifted_tokens(self._h, int(query_id))

    def query_rng_state(self, query_id):
        """The 48-bit state of the query's generator: what its next draw starts from (read-only)"""
        st = C.c_ulonglong(0)
        if not _capi.lib().ifa_engine_query_rng_state(self._h, int(query_id), C.byref(st)):
            raise EngineError(self._err())
        return st.value

    def prefix_cache_stats(self):
        """{active, hits, tokens, copies} of the prompt prefix cache (model_info keys prefix_cache*)"""
        return {k: self.model_info("prefix_cache" + ("_" + k if k != "active" else "")) for k in ("active", "hits", "tokens", "copies")}

    def worker_plan(self, rank):
        """{stage, n_stages, tp_rank, tp_size, layer0, layer1} of partition rank `rank` (None: no such rank)"""
        out = (C.c_int * 6)()
        if _capi.lib().ifa_engine_worker_plan(self._h, int(rank), out) != 0:
            return None
        return dict(zip(("stage", "n_stages", "tp_rank", "tp_size", "layer0", "layer1"), [int(v) for v in out]))

    def worker_tensor(self, rank, layer, tid, expert=-1):
        """(dtype, uint8 host copy, rows, cols) of the slice of tensor (layer local to the rank, tid) rank `rank` holds -- reference
        layout bytes -- or None.  Test surface: the ranks' slices put together are the model the oracle is given."""
        from . import dtypes as dt
        L = _capi.lib()
        h = L.ifa_engine_worker(self._h, int(rank))
        if not h:
            return None
        d, p, r, c = C.c_int(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        if expert >= 0:
            rc = L.ifa_model_get_expert_tensor(C.c_void_p(h), layer, expert, tid, C.byref(d), C.byref(p), C.byref(r), C.byref(c))
        else:
            rc = L.ifa_model_get_tensor(C.c_void_p(h), layer, tid, C.byref(d), C.byref(p), C.byref(r), C.byref(c))
        if rc != 0:
            return None
        nbytes = r.value * dt.row_bytes(d.value, c.value)
        out = np.empty(nbytes, np.uint8)
        _capi.check(L.ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, nbytes, None))
        _capi.check(L.ifa_stream_sync(None))
        return d.value, out, r.value, c.value


def sampling_choose(logits_f16, strategy_id, max_k=8, top_p=0.9, pool_size=50, temperature=1.0, seed=1, n_draws=1):
    """Host-only StdSamplingStrategy::ChooseTokens on one F16 logits row: (drawn ids, their probabilities, pool ids, pool probs)."""
    lg = np.ascontiguousarray(logits_f16, np.float16)
    ids = (C.c_int * max(1, n_draws))(); pr = (C.c_float * max(1, n_draws))()
    pid = (C.c_int * 256)(); ppr = (C.c_float * 256)()
    n = _capi.lib().ifa_sampling_choose(lg.ctypes.data_as(C.c_void_p), lg.size, int(strategy_id), max_k, top_p, pool_size, temperature,
                                        int(seed), n_draws, ids, pr, pid, ppr, 256)
    if n < 0:
        raise EngineError(_capi.lib().ifa_engine_last_error().decode(errors="replace"))
    return [ids[i] for i in range(n_draws)], [pr[i] for i in range(n_draws)], [pid[i] for i in range(min(n, 256))], [ppr[i] for i in range(min(n, 256))]


def prefix_cache_plan(records, busy, stamps, prompt, min_tokens=16):
    """Host-only: the prefix cache's plan for `prompt` over slots holding `records` (lists of token ids): (slot, src_slot, reuse_len),
    src_slot -1 when nothing is copied; None on bad arguments / no free slot (ifa_prefix_cache_plan)."""
    n = len(records)
    flat = [int(t) for r in records for t in r]
    fl = (C.c_int * max(1, len(flat)))(*flat)
    lens = (C.c_int * max(1, n))(*[len(r) for r in records])
    bz = (C.c_int * max(1, n))(*[int(bool(b)) for b in busy])
    st = (C.c_longlong * max(1, n))(*[int(v) for v in stamps])
    pr = (C.c_int * max(1, len(prompt)))(*[int(t) for t in prompt])
    out = (C.c_int * 3)()
    if _capi.lib().ifa_prefix_cache_plan(fl, lens, bz, st, n, pr, len(prompt), int(min_tokens), out) != 0:
        return None
    return out[0], out[1], out[2]


def sampling_choose_ex(logits_f16, strategy_id, temperature=1.0, seed=1, n_draws=1, mu=None, max_k=8, top_p=0.9, pool_size=50, min_p=0.05,
                       z=0.95, typical_p=0.95, eta=0.1, tau=5.0, text=()):
    """Any restated strategy (incl. min_p 7, tfs 8, typical 9, mirostat 10): (ids, probs, pool ids, pool probs, mu after the draws)."""
    lg = np.ascontiguousarray(logits_f16, np.float16)
    params = (C.c_float * 9)(max_k, top_p, pool_size, min_p, z, typical_p, eta, tau, 0)
    ids = (C.c_int * max(1, n_draws))(); pr = (C.c_float * max(1, n_draws))()
    pid = (C.c_int * 256)(); ppr = (C.c_float * 256)()
    m = C.c_float(float("nan") if mu is None else mu)
    txt = (C.c_int * max(1, len(text)))(*[int(t) for t in text])
    n = _capi.lib().ifa_sampling_choose_ex(lg.ctypes.data_as(C.c_void_p), lg.size, int(strategy_id), params, temperature, int(seed), n_draws,
                                           ids, pr, pid, ppr, 256, C.byref(m), txt, len(text))
    if n < 0:
        raise EngineError(_capi.lib().ifa_engine_last_error().decode(errors="replace"))
    return [ids[i] for i in range(n_draws)], [pr[i] for i in range(n_draws)], [pid[i] for i in range(min(n, 256))], [ppr[i] for i in range(min(n, 256))], m.value


def sampling_choose_from_pool(cand_ids, cand_vals_f16, strategy_id, temperature=1.0, seed=1, n_draws=1, mu=None, max_k=8, top_p=0.9, pool_size=50,
                              min_p=0.05, z=0.95, typical_p=0.95, eta=0.1, tau=5.0, text=()):
    """sampling_choose_ex given the row's candidate pool (ids, F16 values, best first: SortedTopK / ifa_topk_pool) instead of the row."""
    cid = np.ascontiguousarray(cand_ids, np.int32).reshape(-1)
    cv = np.ascontiguousarray(cand_vals_f16).view(np.uint16).reshape(-1) if len(cand_vals_f16) else np.zeros(0, np.uint16)
    assert cid.size == cv.size
    params = (C.c_float * 9)(max_k, top_p, pool_size, min_p, z, typical_p, eta, tau, 0)
    ids = (C.c_int * max(1, n_draws))(); pr = (C.c_float * max(1, n_draws))()
    pid = (C.c_int * 256)(); ppr = (C.c_float * 256)()
    m = C.c_float(float("nan") if mu is None else mu)
    txt = (C.c_int * max(1, len(text)))(*[int(t) for t in text])
    n = _capi.lib().ifa_sampling_choose_from_pool(cid.ctypes.data_as(C.POINTER(C.c_int)), cv.ctypes.data_as(C.c_void_p), cid.size, int(strategy_id), params,
                                                  temperature, int(seed), n_draws, ids, pr, pid, ppr, 256, C.byref(m), txt, len(text))
    if n < 0:
        raise EngineError(_capi.lib().ifa_engine_last_error().decode(errors="replace"))
    return [ids[i] for i in range(n_draws)], [pr[i] for i in range(n_draws)], [pid[i] for i in range(min(n, 256))], [ppr[i] for i in range(min(n, 256))], m.value


def random_doubles(seed, n):
    out = (C.c_double * n)()
    _capi.lib().ifa_sampling_random_doubles(int(seed), n, out)
    return [out[i] for i in range(n)]


def context_shift_plan(n_tokens, processed, max_ctx, keep):
    """Host-only: the context shift's policy (ifa_context_shift_plan): None for bad arguments, () for no shift, else (keep, discard)"""
    out = (C.c_int * 2)()
    rc = _capi.lib().ifa_context_shift_plan(int(n_tokens), int(processed), int(max_ctx), int(keep), out)
    return None if rc < 0 else (() if rc == 0 else (out[0], out[1]))
