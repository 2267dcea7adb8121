"""DecodeWorker -- Python handle on the per-device decode worker of the C ABI
(ifa_model_*), the counterpart of the reference's GpuInferenceWorker
(src/transformer/inference_worker.h:23-62).  torch is used only to hold device
memory; all compute happens in libinferflow_amd.so."""
import ctypes as C

import numpy as np

from . import _capi, dtypes as dt
from ._capi import ModelConfig, check, lib

# tensor ids (include/inferflow_amd.h)
T_EMBD, T_OUT_NORM, T_OUT_NORM_B, T_LM_HEAD = 0, 1, 2, 3
T_ATTN_NORM, T_ATTN_NORM_B, T_WQ, T_WK, T_WV, T_WO = 10, 11, 12, 13, 14, 15
T_FFN_NORM, T_FFN_NORM_B, T_W1, T_W2, T_W3, T_MOE_GATE = 16, 17, 18, 19, 20, 21
T_WQ_B, T_WK_B, T_WV_B, T_WO_B, T_W1_B, T_W2_B, T_W3_B = 22, 23, 24, 25, 26, 27, 28
T_ATTN_POST_NORM, T_ATTN_POST_NORM_B, T_FFN_POST_NORM, T_FFN_POST_NORM_B = 29, 30, 31, 32      # self_attn.post_norm / feed_forward.post_norm

_DEFAULTS = dict(norm_kind=0, act_kind=0, is_glu=1, rope_order=2, use_alibi=0, parallel_attn=0, share_input=0,
                 rope_theta=10000.0, partial_rotary=1.0, kq_scale=1.0, eps=1e-5, kv_dtype=dt.F16,
                 full_quant_gemv=1, experts=0, moe_top_k=0, moe_norm_topk=1, tp_rank=0, tp_size=1, device=0,
                 attn_norm_base=0.0, ffn_norm_base=0.0, out_norm_base=0.0, attn_out_scale=1.0, ffn_out_scale=1.0, out_scale=1.0,
                 embd_scale=0.0)


class DecodeWorker:
    def __init__(self, **kw):
        cfg = ModelConfig()
        vals = dict(_DEFAULTS)
        vals.update(kw)
        for k, v in vals.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self._h = C.c_void_p()
        check(lib().ifa_model_create(C.byref(cfg), C.byref(self._h)))

    # ---- weights -----------------------------------------------------------
    def set_tensor(self, layer, tid, dtype, dev_tensor, rows, cols, expert=-1):
        """dev_tensor: torch cuda tensor holding reference-layout blocks (uint8) or F16 values.
        expert >= 0: the W1/W2/W3 of one MoE expert of that layer."""
        check(lib().ifa_model_set_tensor(self._h, layer, tid, expert, dtype, C.c_void_p(dev_tensor.data_ptr()), rows, cols))

    def set_tensor_f16(self, layer, tid, target_dtype, dev_f16, rows=None, cols=None, expert=-1):
        if rows is None:
            rows, cols = (1, dev_f16.numel()) if dev_f16.dim() == 1 else dev_f16.shape
        check(lib().ifa_model_set_tensor_f16(self._h, layer, tid, expert, target_dtype,
                                             C.c_void_p(dev_f16.data_ptr()), rows, cols))

    def finalize(self):
        check(lib().ifa_model_finalize(self._h))

    def reset(self):
        check(lib().ifa_model_reset(self._h))

    def set_option(self, name, value):
        check(lib().ifa_model_set_option(self._h, name.encode(), int(value)))

    def perf_stat(self, clear=True):
        """{key: ms} of option perf_stat in the reference's InferencePerfStat key space (include/inferflow_amd.h: ifa_model_perf_stat)"""
        keys, ms, n = np.zeros(256, np.int32), np.zeros(256, np.float32), C.c_int(0)
        check(lib().ifa_model_perf_stat(self._h, keys.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p), 256, C.byref(n), 1 if clear else 0))
        return {int(k): float(v) for k, v in zip(keys[:min(n.value, 256)], ms[:min(n.value, 256)])}

    def set_excluded_tokens(self, ids):
        """ids (<= 3) the greedy argmax never selects (unk / Invalid-type tokens, sampling_strategy.cc:281-297)"""
        a = np.ascontiguousarray(ids, np.int32)
        check(lib().ifa_model_set_excluded_tokens(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def fused_supported(self):
        buf = C.create_string_buffer(256)
        ok = lib().ifa_model_fused_supported(self._h, buf, 256)
        return bool(ok), buf.value.decode()

    # ---- inference -----------------------------------------------------------
    def forward(self, tokens, prefix_len, logits_out=None):
        """One Infer() step (op-by-op).  logits_out: optional torch cuda f16 [T][vocab]."""
        toks = np.ascontiguousarray(tokens, np.int32)
        nxt = C.c_int(0)
        check(lib().ifa_model_forward(self._h, toks.ctypes.data_as(C.c_void_p), toks.size, prefix_len,
                                      C.c_void_p(logits_out.data_ptr()) if logits_out is not None else None,
                                      C.byref(nxt)))
        return nxt.value

    def kv_slots(self, n):
        """Independent KV caches, one per concurrent query (slot 0 exists after finalize)."""
        check(lib().ifa_model_kv_slots(self._h, int(n)))

    def select_kv(self, slot):
        check(lib().ifa_model_select_kv(self._h, int(slot)))

    def kv_copy(self, src, dst, n_rows):
        """Cache rows [0, n_rows) of every layer's K and V from slot src to slot dst: one launch on the worker's stream, enqueue-only."""
        check(lib().ifa_model_kv_copy(self._h, int(src), int(dst), int(n_rows)))

    def kv_shift(self, slot, keep, discard, n_rows):
        """Context shift on query slot `slot`: rows [keep, keep + discard) of its n_rows cache rows are dropped, the rows behind them
        move down and the moved K rows are rotated back by `discard` positions (ifa_model_kv_shift); enqueue-only."""
        check(lib().ifa_model_kv_shift(self._h, int(slot), int(keep), int(discard), int(n_rows)))

    def kv_shift_rows(self, kcache_ptr, vcache_ptr, table_ptr, keep, discard, n_rows):
        """ifa_kv_shift_rows with this worker's cache geometry and stream on one layer's pair of device buffers (addresses; None skips
        a side): table_ptr = head_dim / 2 fp32 (c, s) pairs on the device.  Enqueue-only."""
        c = self.cfg
        kv_shift_rows(c.kv_dtype, kcache_ptr, vcache_ptr, c.kv_heads, c.head_dim, c.rope_order, int(c.head_dim * c.partial_rotary + 0.5), table_ptr,
                      keep, discard, n_rows, lib().ifa_model_stream(self._h))

    def sync(self):
        """Wait for everything enqueued on the worker's stream (kv_copy only enqueues; forward / decode synchronise themselves)."""
        check(lib().ifa_stream_sync(C.c_void_p(lib().ifa_model_stream(self._h))))

    def decode_batch(self, tokens, positions, slots, logits_out=None):
        """One new token for each of n queries (dynamic batching); returns the n greedy next tokens."""
        toks = np.ascontiguousarray(tokens, np.int32)
        pos = np.ascontiguousarray(positions, np.int32)
        sl = np.ascontiguousarray(slots, np.int32)
        out = np.zeros(toks.size, np.int32)
        check(lib().ifa_model_decode_batch(self._h, toks.size, toks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                           sl.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(logits_out.data_ptr()) if logits_out is not None else None))
        return out

    def decode_batch_steps(self, tokens, positions, slots, n_steps, rows=None, timed=False):
        """n_steps device-fed batched steps of the same rows with one synchronisation (ifa_model_decode_batch_steps).  rows: None (all
        greedy, no stop ids) or one dict per row with any of strategy (SampleParams-style tuple (strategy_id, temperature, top_p, max_k,
        min_p), default greedy), pool_size (default 1), rng_state, state_slot (default -1), stop_ids (at most 8).
        Returns (tokens int32 [n_steps][n] with -1 where a row was frozen, emitted int32 [n], generator states [n], gpu_ms)."""
        from ._capi import BatchRow
        toks = np.ascontiguousarray(tokens, np.int32)
        pos = np.ascontiguousarray(positions, np.int32)
        sl = np.ascontiguousarray(slots, np.int32)
        n = toks.size
        arr = None
        if rows is not None:
            assert len(rows) == n
            arr = (BatchRow * n)()
            for r, d in enumerate(rows):
                b = arr[r]
                b.struct_size = C.sizeof(BatchRow)
                sid, temp, top_p, max_k, min_p = d.get("strategy", (2, 1.0, 1.0, 1, 0.0))
                b.p.strategy_id, b.p.temperature, b.p.top_p, b.p.max_k, b.p.min_p = int(sid), float(temp), float(top_p), int(max_k), float(min_p)
                b.p.pool_size = int(d.get("pool_size", 1))
                b.state_slot = int(d.get("state_slot", -1))
                b.rng_state = int(d.get("rng_state", 0))
                stops = list(d.get("stop_ids", ()))
                b.n_stop = len(stops)
                for i, t in enumerate(stops[:8]):
                    b.stop_ids[i] = int(t)
        out = np.full((int(n_steps), n), -2, np.int32)
        emitted = np.full(n, -2, np.int32)
        ms = C.c_float(-1.0)
        check(lib().ifa_model_decode_batch_steps(self._h, n, toks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p),
                                                 int(n_steps), arr, out.ctypes.data_as(C.c_void_p), emitted.ctypes.data_as(C.c_void_p),
                                                 C.byref(ms) if timed else None))
        states = [int(arr[r].rng_state) for r in range(n)] if arr is not None else [0] * n
        return out, emitted, states, ms.value

    def decode_draft(self, tokens, pos0, logits_out=None):
        """The draft step on the selected KV slot: row i is tokens[i] at position pos0 + i behind rows [0, pos0 + i) -- tokens[0] the
        last committed token, the rest draft tokens (2..8 rows).  Returns the greedy next token of every row."""
        toks = np.ascontiguousarray(tokens, np.int32)
        out = np.zeros(toks.size, np.int32)
        check(lib().ifa_model_decode_draft(self._h, toks.size, toks.ctypes.data_as(C.c_void_p), int(pos0), out.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(logits_out.data_ptr()) if logits_out is not None else None))
        return out

    def decode_draft_sampled(self, tokens, pos0, params, rng_state, state_slot=-1):
        """The draft step for a seeded sampled query (ifa_model_decode_draft_sampled): decode_draft's rows, drawn as a chain on the
        device.  params: _capi.SampleParams (pool_size = the step's pool length); rng_state: the query's generator state; state_slot:
        the logit-processor slot, -1 for none.  Returns (emitted tokens int32 [n_out], generator state afterwards)."""
        toks = np.ascontiguousarray(tokens, np.int32)
        out = np.full(toks.size, -2, np.int32)
        st, n_out = C.c_ulonglong(int(rng_state)), C.c_int(0)
        check(lib().ifa_model_decode_draft_sampled(self._h, toks.size, toks.ctypes.data_as(C.c_void_p), int(pos0), C.byref(params), C.byref(st),
                                                   int(state_slot), out.ctypes.data_as(C.c_void_p), C.byref(n_out)))
        assert np.all(out[n_out.value:] == -1), out
        return out[:n_out.value].copy(), st.value

    def decode(self, first_token, start_pos, n_steps, timed=True):
        """Greedy batch-1 decode with the fused kernels; returns (tokens, gpu_ms)."""
        out = np.zeros(n_steps, np.int32)
        ms = C.c_float(-1.0)
        check(lib().ifa_model_decode(self._h, int(first_token), int(start_pos), int(n_steps),
                                     out.ctypes.data_as(C.c_void_p), C.byref(ms) if timed else None))
        return out, ms.value

    def decode_sampled(self, first_token, start_pos, n_steps, params, rng_state, state_slot=-1, timed=True):
        """decode() with every token drawn on the device (ifa_model_decode_sampled).  params: _capi.SampleParams (pool_size = the
        step's pool length); rng_state: the 48-bit generator state the first draw starts from (rng_state_of_seed); state_slot: the
        logit-processor slot, -1 for none.  Returns (tokens, generator state behind the last draw, gpu_ms)."""
        out = np.zeros(n_steps, np.int32)
        ms = C.c_float(-1.0)
        st = C.c_ulonglong(int(rng_state))
        check(lib().ifa_model_decode_sampled(self._h, int(first_token), int(start_pos), int(n_steps), C.byref(params), C.byref(st), int(state_slot),
                                             out.ctypes.data_as(C.c_void_p), C.byref(ms) if timed else None))
        return out, st.value, ms.value

    def set_pool_excluded(self, ids):
        """ids (any count) the device candidate pool never offers; an empty list clears the mask"""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        check(lib().ifa_model_set_pool_excluded(self._h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size))

    def decode_pool(self, token, pos, k):
        """One decode step that ends in the candidate pool of its logits row (ifa_model_decode_pool).
        Returns (greedy next token, pool ids int32 [count], pool values as F16 bits uint16 [count]), best first."""
        ids, vals = np.zeros(k, np.int32), np.zeros(k, np.uint16)
        nxt, cnt = C.c_int(-1), C.c_int(0)
        check(lib().ifa_model_decode_pool(self._h, int(token), int(pos), int(k), C.byref(nxt), ids.ctypes.data_as(C.c_void_p),
                                          vals.ctypes.data_as(C.c_void_p), C.byref(cnt)))
        return nxt.value, ids[:cnt.value].copy(), vals[:cnt.value].copy()

    def forward_pool(self, tokens, prefix_len, k, logits_out=None):
        """One prompt step (forward) that ends in the candidate pool of its LAST row; returns like decode_pool.
        logits_out: optional torch cuda f16 [T][vocab], as in forward()."""
        toks = np.ascontiguousarray(tokens, np.int32)
        ids, vals = np.zeros(k, np.int32), np.zeros(k, np.uint16)
        nxt, cnt = C.c_int(-1), C.c_int(0)
        check(lib().ifa_model_forward_pool(self._h, toks.ctypes.data_as(C.c_void_p), toks.size, int(prefix_len),
                                           C.c_void_p(logits_out.data_ptr()) if logits_out is not None else None, int(k), C.byref(nxt),
                                           ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), C.byref(cnt)))
        return nxt.value, ids[:cnt.value].copy(), vals[:cnt.value].copy()

    def decode_batch_pool(self, tokens, positions, slots, k, rows_sel):
        """decode_batch whose rows rows_sel (ascending indices into the step's rows) end in their candidate pools.
        Returns (next tokens [n], [(ids, F16 bits)] per selected row)."""
        toks = np.ascontiguousarray(tokens, np.int32)
        pos = np.ascontiguousarray(positions, np.int32)
        sl = np.ascontiguousarray(slots, np.int32)
        sel = np.ascontiguousarray(rows_sel, np.int32).reshape(-1)
        out = np.zeros(toks.size, np.int32)
        ids, vals = np.zeros((max(sel.size, 1), k), np.int32), np.zeros((max(sel.size, 1), k), np.uint16)
        cnt = np.zeros(max(sel.size, 1), np.int32)
        check(lib().ifa_model_decode_batch_pool(self._h, toks.size, toks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                                sl.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(k),
                                                sel.ctypes.data_as(C.c_void_p), sel.size, ids.ctypes.data_as(C.c_void_p),
                                                vals.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
        return out, [(ids[j, :cnt[j]].copy(), vals[j, :cnt[j]].copy()) for j in range(sel.size)]

    def pool_lse(self, cap=256):
        """The log-sum-exp of every row the LAST pool step pooled (option "pool_lse" = 1; empty with it off): float32 [n_sel].
        log p(pool id) = float(pool value) - lse."""
        out, n = np.zeros(cap, np.float32), C.c_int(0)
        check(lib().ifa_model_pool_lse(self._h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def decode_pool_lse(self, token, pos, k):
        """decode_pool with the row's log-sum-exp (sets option "pool_lse" for this step): (next, ids, F16 bits, lse)"""
        self.set_option("pool_lse", 1)
        try:
            nxt, ids, vals = self.decode_pool(token, pos, k)
            return nxt, ids, vals, float(self.pool_lse()[0])
        finally:
            self.set_option("pool_lse", 0)

    def forward_pool_lse(self, tokens, prefix_len, k, logits_out=None):
        """forward_pool with the last row's log-sum-exp: (next, ids, F16 bits, lse)"""
        self.set_option("pool_lse", 1)
        try:
            nxt, ids, vals = self.forward_pool(tokens, prefix_len, k, logits_out)
            return nxt, ids, vals, float(self.pool_lse()[0])
        finally:
            self.set_option("pool_lse", 0)

    def decode_batch_pool_lse(self, tokens, positions, slots, k, rows_sel):
        """decode_batch_pool with the selected rows' log-sum-exp: (next tokens, pools, lse float32 [n_sel])"""
        self.set_option("pool_lse", 1)
        try:
            out, pools = self.decode_batch_pool(tokens, positions, slots, k, rows_sel)
            return out, pools, self.pool_lse(max(len(pools), 1))
        finally:
            self.set_option("pool_lse", 0)

    def logit_state_reset(self, kv_slot, prompt, rep=1.0, freq=0.0, pres=0.0, bias=None):
        """The logit-processor state of the query in kv_slot (ifa_model_logit_state_reset): cleared, the prompt ids marked, the
        penalties and the logit_bias ({id: value}, -inf bans) stored."""
        pr = np.ascontiguousarray(prompt, np.int32).reshape(-1)
        items = sorted((bias or {}).items())
        ids = np.ascontiguousarray([k for k, _ in items], np.int32)
        vals = np.ascontiguousarray([v for _, v in items], np.float32)
        check(lib().ifa_model_logit_state_reset(self._h, int(kv_slot), pr.ctypes.data_as(C.c_void_p) if pr.size else None, pr.size, float(rep), float(freq),
                                                float(pres), ids.ctypes.data_as(C.c_void_p) if ids.size else None,
                                                vals.ctypes.data_as(C.c_void_p) if vals.size else None, ids.size))

    def logit_state_add(self, kv_slots, tokens):
        """One more generated occurrence for every (kv slot, token) pair; enqueue-only (ifa_model_logit_state_add)"""
        sl = np.ascontiguousarray(kv_slots, np.int32).reshape(-1)
        tk = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        assert sl.size == tk.size
        check(lib().ifa_model_logit_state_add(self._h, sl.size, sl.ctypes.data_as(C.c_void_p), tk.ctypes.data_as(C.c_void_p)))

    def pool_adjust(self, state_slots):
        """Arms the NEXT pool step: entry j = the state slot whose processors rewrite pooled row j, -1 = the row stays raw"""
        sl = np.ascontiguousarray(state_slots, np.int32).reshape(-1)
        check(lib().ifa_model_pool_adjust(self._h, sl.size, sl.ctypes.data_as(C.c_void_p) if sl.size else None))

    def forward_score(self, tokens, prefix_len, targets):
        """A scoring prompt (ifa_model_forward_score): per row the log-sum-exp of its logits and its logit at targets[i] (NaN for a
        target below 0), without a [T][vocab] block leaving the worker.  Returns (next token, lse float32 [T], target logit float32 [T]);
        log p(targets[i] | tokens[:i + 1]) = target_logit[i] - lse[i]."""
        toks = np.ascontiguousarray(tokens, np.int32)
        tg = np.ascontiguousarray(targets, np.int32).reshape(-1)
        assert tg.size == toks.size, (tg.size, toks.size)
        lse, tl = np.zeros(toks.size, np.float32), np.zeros(toks.size, np.float32)
        nxt = C.c_int(-1)
        check(lib().ifa_model_forward_score(self._h, toks.ctypes.data_as(C.c_void_p), toks.size, int(prefix_len), tg.ctypes.data_as(C.c_void_p),
                                            lse.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), C.byref(nxt)))
        return nxt.value, lse, tl

    def decode_prepare(self, start_pos, n_steps):
        """Set up (capture) what decode(., start_pos, n_steps) replays, without running a step."""
        check(lib().ifa_model_decode_prepare(self._h, int(start_pos), int(n_steps)))

    def time_kernel(self, which, iters=200):
        """avg microseconds per launch of one fused kernel (0 qkv, 1 attn, 2 wo, 3 ffn13, 4 w2, 5 lm_head)"""
        us = C.c_float(0)
        check(lib().ifa_model_time_kernel(self._h, which, iters, C.byref(us)))
        return us.value

    ROUTE_FIELDS = ("kind", "nsplits", "pb", "kt", "ul", "gk", "rw", "chain", "split_threshold", "split", "lds_attn", "lds_scores", "lds_pv",
                    "error", "num_cus", "visible_cus", "waits")
    ROUTE_KINDS = ("one_workgroup", "split", "fused_tail")

    def decode_route(self):
        """the plan of the last decode / decode_prepare call (csrc/ifa_decode_route.h) as a dict; kind as one of ROUTE_KINDS"""
        out = (C.c_int * len(self.ROUTE_FIELDS))()
        check(lib().ifa_model_decode_route(self._h, out, len(out)))
        d = dict(zip(self.ROUTE_FIELDS, out))
        d["kind"] = self.ROUTE_KINDS[d["kind"]]
        return d

    GEMV_PLAN_FIELDS = ("kind", "nj", "nchunk", "njl", "rw", "threads", "np", "grid", "waves", "npass", "partial", "lds", "error")
    GEMV_MODEL_FIELDS = GEMV_PLAN_FIELDS + ("single", "dtype", "epi", "norm", "cols", "total_rows", "num_cus", "launches")
    GEMV_KINDS = ("none", "classic", "long", "f16x")
    GEMV_ROLES = ("qkv", "wo", "ffn13", "w2")

    def gemv_plan(self, layer, role):
        """what the fused GEMV launch of `role` (one of GEMV_ROLES) of a layer would run if the step were enqueued now
        (csrc/ifa_decode_gemv_plan.h) as a dict; kind as one of GEMV_KINDS; single = 0: the step would not run this launch on its own"""
        out = (C.c_int * len(self.GEMV_MODEL_FIELDS))()
        check(lib().ifa_model_gemv_plan(self._h, int(layer), self.GEMV_ROLES.index(role), out, len(out)))
        d = dict(zip(self.GEMV_MODEL_FIELDS, out))
        d["kind"] = self.GEMV_KINDS[d["kind"]]
        return d

    PROMPT_ROUTE_FIELDS = ("kind", "first_pass", "norm_fused", "res_mid") + tuple(
        p + "_" + k for p in ("qkv", "wo", "w13", "w2") for k in ("kernel", "src", "mo", "no_waits")) + ("need_mo", "need_x32")
    PROMPT_ROUTE_KINDS = ("exact", "op_by_op", "rows", "mid", "big")

    def prompt_route(self):
        """the route of the last prompt call (csrc/ifa_prompt_route.h) as a dict; kind as one of PROMPT_ROUTE_KINDS"""
        out = (C.c_int * len(self.PROMPT_ROUTE_FIELDS))()
        check(lib().ifa_model_prompt_route(self._h, out, len(out)))
        d = dict(zip(self.PROMPT_ROUTE_FIELDS, out))
        d["kind"] = self.PROMPT_ROUTE_KINDS[d["kind"]]
        return d

    def moe_plan(self, layer, T, caller_norm=0):
        """what an MoE layer would run over T rows now (csrc/ifa_moe_plan.h) as a dict of MOE_PLAN_FIELDS; kind as one of MOE_KINDS, router
        as one of MOE_ROUTERS.  caller_norm: the fused batched step's call (norm and residual left to the layer)"""
        out = (C.c_int * len(MOE_PLAN_FIELDS))()
        check(lib().ifa_model_moe_plan(self._h, int(layer), int(T), int(caller_norm), out, len(out)))
        return _moe_plan_dict(out)

    def get_tensor_host(self, layer, tid):
        """(dtype, uint8/uint16 numpy copy, rows, cols) of a loaded tensor in reference layout, or None."""
        d, p, r, c = C.c_int(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        rc = lib().ifa_model_get_tensor(self._h, layer, tid, C.byref(d), C.byref(p), C.byref(r), C.byref(c))
        if rc == 1:
            return None
        check(rc)
        nbytes = r.value * dt.row_bytes(d.value, c.value)
        out = np.empty(nbytes, np.uint8)
        check(lib().ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, nbytes, None))
        check(lib().ifa_stream_sync(None))
        if d.value == dt.F16:
            out = out.view(np.uint16)
        return d.value, out, r.value, c.value

    def get_expert_tensor_host(self, layer, expert, tid):
        """(dtype, uint8 copy, rows, cols) of W1 / W2 / W3 of one expert of an MoE layer in reference layout, or None"""
        d, p, r, c = C.c_int(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        rc = lib().ifa_model_get_expert_tensor(self._h, layer, expert, tid, C.byref(d), C.byref(p), C.byref(r), C.byref(c))
        if rc == 1:
            return None
        check(rc)
        nbytes = r.value * dt.row_bytes(d.value, c.value)
        out = np.empty(nbytes, np.uint8)
        check(lib().ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, nbytes, None))
        check(lib().ifa_stream_sync(None))
        return d.value, out, r.value, c.value

    # ---- tensor-parallel segments (enqueue only; the caller all-reduces in between) ----
    def set_stream(self, stream_ptr):
        check(lib().ifa_model_set_stream(self._h, C.c_void_p(stream_ptr)))

    def tp_begin(self, token, pos):
        check(lib().ifa_model_tp_begin(self._h, int(token), int(pos)))

    def tp_begin_hidden(self, x_dev_f16, pos):
        check(lib().ifa_model_tp_begin_hidden(self._h, C.c_void_p(x_dev_f16.data_ptr()), int(pos)))

    def tp_hidden(self, x_out_dev_f16):
        check(lib().ifa_model_tp_hidden(self._h, C.c_void_p(x_out_dev_f16.data_ptr())))

    def tp_attn(self, layer, partial):
        check(lib().ifa_model_tp_attn(self._h, layer, C.c_void_p(partial.data_ptr())))

    def tp_post_attn(self, layer, reduced):
        check(lib().ifa_model_tp_post_attn(self._h, layer, C.c_void_p(reduced.data_ptr())))

    def tp_ffn(self, layer, partial):
        check(lib().ifa_model_tp_ffn(self._h, layer, C.c_void_p(partial.data_ptr())))

    def tp_post_ffn(self, layer, reduced):
        check(lib().ifa_model_tp_post_ffn(self._h, layer, C.c_void_p(reduced.data_ptr())))

    def tp_logits(self, shard_out):
        check(lib().ifa_model_tp_logits(self._h, C.c_void_p(shard_out.data_ptr())))

    def tp_set_token(self, token_dev_int32):
        check(lib().ifa_model_tp_set_token(self._h, C.c_void_p(token_dev_int32.data_ptr())))

    def buffer(self, name, layer=0):
        p, n = C.c_void_p(), C.c_size_t()
        check(lib().ifa_model_get_buffer(self._h, name.encode(), layer, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_buffer(self, name, layer=0, nbytes=None):
        p, n = self.buffer(name, layer)
        n = n if nbytes is None else nbytes
        out = np.empty(n, np.uint8)
        check(lib().ifa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), n, None))
        check(lib().ifa_stream_sync(None))
        return out

    def write_buffer(self, name, data, layer=0, offset=0):
        """host bytes -> a worker buffer (debug surface of the layer-wise parity tests: the layer input "x", K / V cache rows)"""
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        p, n = self.buffer(name, layer)
        assert offset + a.size <= n, (name, offset, a.size, n)
        check(lib().ifa_memcpy_h2d(C.c_void_p(p + offset), a.ctypes.data_as(C.c_void_p), a.size, None))
        check(lib().ifa_stream_sync(None))

    def close(self):
        if self._h:
            lib().ifa_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topk_pool(logits, k, excluded_bits=None, stream=None):
    """ifa_topk_pool over a torch cuda F16 tensor [rows][n] (or [n]): the k best (value, id) pairs per row, best first, lower id
    among equal values, NaN and the ids of excluded_bits (torch cuda int32 bitmask, ceil(n / 32) words) never offered.
    Returns torch cuda tensors (ids int32 [rows][k], values int16 = F16 bits [rows][k], counts int32 [rows]); enqueue-only."""
    import torch
    rows, n = (1, logits.numel()) if logits.dim() == 1 else logits.shape
    ids = torch.empty((rows, max(k, 1)), dtype=torch.int32, device=logits.device)
    vals = torch.empty((rows, max(k, 1)), dtype=torch.int16, device=logits.device)
    cnt = torch.empty(rows, dtype=torch.int32, device=logits.device)
    check(lib().ifa_topk_pool(C.c_void_p(logits.data_ptr()), rows, n, int(k),
                              C.c_void_p(excluded_bits.data_ptr()) if excluded_bits is not None else None,
                              C.c_void_p(ids.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(stream)))
    return ids, vals, cnt


def gemv_plan(dtype, epi, norm, cols, total_rows, num_cus=256, rpw=0, x_add=0):
    """ifa_decode_gemv_plan: the pure launch plan of the fused decode GEMV (no device) as a dict of DecodeWorker.GEMV_PLAN_FIELDS"""
    facts = (C.c_int * 8)(int(dtype), int(epi), int(norm), int(x_add), int(cols), int(total_rows), int(num_cus), int(rpw))
    out = (C.c_int * len(DecodeWorker.GEMV_PLAN_FIELDS))()
    check(lib().ifa_decode_gemv_plan(facts, 8, out, len(out)))
    d = dict(zip(DecodeWorker.GEMV_PLAN_FIELDS, out))
    d["kind"] = DecodeWorker.GEMV_KINDS[d["kind"]]
    return d


GEMM_ROWS_FACTS = ("T", "nsets", "rows0", "rows1", "rows2", "nblk", "epi", "norm", "mo", "has_w1", "no_waits", "waits_on", "num_cus", "visible_cus",
                   "wgs_per_cu", "kparts_off", "kparts_min")
GEMM_ROWS_TRY = ("kparts", "kpm", "tiles", "groups", "grid", "lds", "scratch")
GEMM_ROWS_RECORD = ("T", "total_rows", "nblk", "epi", "norm", "mo", "tx", "ch", "nchunk", "n_try", "attempt") + GEMM_ROWS_TRY + (
    "declined_grid", "occupancy", "visible_cus", "waits_on", "err_word")


def gemm_rows_plan(T, rows, cols, epi=0, norm=0, mo=1, num_cus=256, visible_cus=None, **over):
    """ifa_gemm_rows_plan: the pure launch plan of the rows GEMM (csrc/ifa_gemm_rows_plan.h, no device) as a dict: error, total_rows,
    ntiles, tx, ch, chunk_cols, nchunk, tries = [dict of GEMM_ROWS_TRY] in the order they are tried.  rows: the rows of the 1..3 sets."""
    rows = tuple(rows) + (0,) * (3 - len(tuple(rows)))
    f = dict(T=T, nsets=len([r for r in rows if r]) or 1, rows0=rows[0], rows1=rows[1], rows2=rows[2], nblk=cols // 32, epi=epi, norm=norm, mo=mo,
             has_w1=1, no_waits=0, waits_on=1, num_cus=num_cus, visible_cus=num_cus if visible_cus is None else visible_cus, wgs_per_cu=0,
             kparts_off=0, kparts_min=0)
    f.update(over)
    facts = (C.c_int * len(GEMM_ROWS_FACTS))(*[int(f[k]) for k in GEMM_ROWS_FACTS])
    out = (C.c_int * 22)()
    check(lib().ifa_gemm_rows_plan(facts, len(GEMM_ROWS_FACTS), out, 22))
    v = list(out)
    d = dict(zip(("error", "total_rows", "ntiles", "tx", "ch", "chunk_cols", "nchunk"), v[:7]))
    d["tries"] = [dict(zip(GEMM_ROWS_TRY, v[8 + 7 * i:15 + 7 * i])) for i in range(v[7])]
    return d


MOE_FACTS = ("T", "experts", "top_k", "dim", "ffn", "w_dtype", "w_ax8", "w_q4", "full_quant_gemv", "norm_kind", "gate_f16", "gate_cols_match",
             "has_ffn_norm", "experts_uniform", "have_table", "have_table_aos", "have_table_mo", "moe_device", "moe_router_fused", "moe_singles",
             "moe_overlap", "gemm_rows", "rows_mo", "rows_use_mfma", "rows_mfma_ok", "rows_q4_ok", "singles_ok", "caller_norm")
MOE_PLAN_FIELDS = ("kind", "router", "device_ok", "cap", "tile_rows", "small_max", "max_tiles", "max_singles", "max_smalls", "rows_kernel",
                   "rows_mfma", "smalls_mo", "side_stream", "host_sync")
MOE_KINDS = ("host", "device_grouped", "device_singles")
MOE_ROUTERS = ("ops", "fused")


def _moe_plan_dict(out):
    d = dict(zip(MOE_PLAN_FIELDS, out))
    d["kind"] = MOE_KINDS[d["kind"]]
    d["router"] = MOE_ROUTERS[d["router"]]
    return d


def moe_plan(**facts):
    """ifa_moe_plan: the pure plan of a mixture-of-experts layer (csrc/ifa_moe_plan.h, no device) from all of MOE_FACTS, as a dict of
    MOE_PLAN_FIELDS; kind as one of MOE_KINDS, router as one of MOE_ROUTERS"""
    if set(facts) != set(MOE_FACTS):
        raise KeyError("moe_plan: facts %s missing, %s unknown" % (sorted(set(MOE_FACTS) - set(facts)), sorted(set(facts) - set(MOE_FACTS))))
    f = (C.c_int * len(MOE_FACTS))(*[int(facts[k]) for k in MOE_FACTS])
    out = (C.c_int * len(MOE_PLAN_FIELDS))()
    check(lib().ifa_moe_plan(f, len(MOE_FACTS), out, len(out)))
    return _moe_plan_dict(out)


def gemm_rows_launches():
    """ifa_gemm_rows_launches: (records, launches since the last read); records: the last (at most 8) rows GEMM launches of this process,
    oldest first, as dicts of GEMM_ROWS_RECORD.  Reading clears them."""
    n = len(GEMM_ROWS_RECORD)
    out = (C.c_int * (2 + 8 * n))()
    check(lib().ifa_gemm_rows_launches(out, len(out)))
    v = list(out)
    return [dict(zip(GEMM_ROWS_RECORD, v[2 + i * n:2 + (i + 1) * n])) for i in range(v[0])], v[1]


def rng_state_of_seed(seed):
    """the 48-bit state of the java.util.Random generator right after seeding it with `seed`"""
    return (int(seed) ^ 0x5DEECE66D) & ((1 << 48) - 1)


def sample_params_array(rows):
    """numpy structured array [len(rows)] laid out like ifa_sample_params from (strategy_id, temperature, top_p, max_k, min_p) tuples"""
    rec = np.dtype([("strategy_id", np.int32), ("temperature", np.float32), ("top_p", np.float32), ("max_k", np.int32), ("min_p", np.float32),
                   ("pool_size", np.int32)])
    a = np.zeros(len(rows), rec)
    for i, r in enumerate(rows):
        a[i] = tuple(r) + (0,)
    return a


def sample_pool_host(ids, vals_f16_bits, params, rng_state):
    """ifa_sample_pool_host on one pool (no device): ids int32 [count], vals uint16 F16 bits [count], params a row of
    sample_params_array (or _capi.SampleParams).  Returns (token, index, cut length, weights float32 [count], sorted ids int32 [count],
    generator state afterwards); raises IfaError for an empty pool."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    vals = np.ascontiguousarray(vals_f16_bits).view(np.uint16).reshape(-1)
    assert ids.size == vals.size
    if isinstance(params, np.void):
        params = np.array([params], params.dtype)
    pp = C.c_void_p(params.ctypes.data) if isinstance(params, np.ndarray) else C.cast(C.pointer(params), C.c_void_p)
    st = C.c_ulonglong(int(rng_state))
    tok, idx, cut = C.c_int(-1), C.c_int(-1), C.c_int(0)
    w, order = np.zeros(max(ids.size, 1), np.float32), np.full(max(ids.size, 1), -1, np.int32)
    check(lib().ifa_sample_pool_host(ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), ids.size, pp, C.cast(C.pointer(st), C.c_void_p),
                                     C.cast(C.pointer(tok), C.c_void_p), C.cast(C.pointer(idx), C.c_void_p), C.cast(C.pointer(cut), C.c_void_p),
                                     w.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p)))
    return tok.value, idx.value, cut.value, w[:ids.size], order[:ids.size], st.value


def sample_pool_rows(counts, ids, vals, params, rng_states, err, weights=None, stream=None):
    """ifa_sample_pool_rows on torch cuda tensors: counts int32 [rows], ids int32 / vals int16 F16 bits [rows][k], params uint8 bytes of
    a sample_params_array [rows], rng_states int64 [rows] (advance in place), err int32 [1]; weights float32 [rows][k] or None.
    Returns (tokens int32 [rows], index int32 [rows]); enqueue-only."""
    import torch
    rows, k = ids.shape
    tokens = torch.empty(rows, dtype=torch.int32, device=ids.device)
    index = torch.empty(rows, dtype=torch.int32, device=ids.device)
    check(lib().ifa_sample_pool_rows(_ptr(counts), _ptr(ids), _ptr(vals), rows, int(k), _ptr(params), _ptr(rng_states), _ptr(tokens), _ptr(index),
                                     _ptr(weights), _ptr(err), C.c_void_p(stream)))
    return tokens, index


def sample_verify_host(counts, ids, vals_f16_bits, params, draft, rng_state, err=0):
    """ifa_sample_verify_host (no device): the rows of a draft step drawn as a chain.  counts int32 [rows], ids int32 / vals uint16
    F16 bits [rows][k], params a row of sample_params_array (or _capi.SampleParams), draft int32 [rows - 1] (draft[i]: the guess for
    the token row i emits), rng_state the query's generator state, err the error word's value before the call.
    Returns (tokens int32 [rows], index int32 [rows], n_out, generator state afterwards, err)."""
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    ids = np.ascontiguousarray(ids, np.int32)
    vals = np.ascontiguousarray(vals_f16_bits).view(np.uint16)
    rows, k = ids.shape
    assert counts.size == rows and vals.shape == ids.shape
    draft = np.ascontiguousarray(draft, np.int32).reshape(-1)
    assert draft.size >= rows - 1
    if isinstance(params, np.void):
        params = np.array([params], params.dtype)
    pp = C.c_void_p(params.ctypes.data) if isinstance(params, np.ndarray) else C.cast(C.pointer(params), C.c_void_p)
    st, n_out, e = C.c_ulonglong(int(rng_state)), C.c_int(-1), C.c_int(int(err))
    tokens, index = np.full(rows, -2, np.int32), np.full(rows, -2, np.int32)
    check(lib().ifa_sample_verify_host(counts.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), rows, int(k), pp,
                                       draft.ctypes.data_as(C.c_void_p) if draft.size else None, C.cast(C.pointer(st), C.c_void_p),
                                       tokens.ctypes.data_as(C.c_void_p), index.ctypes.data_as(C.c_void_p), C.cast(C.pointer(n_out), C.c_void_p),
                                       C.cast(C.pointer(e), C.c_void_p)))
    return tokens, index, n_out.value, st.value, e.value


def sample_verify_rows(counts, ids, vals, params, draft, rng_state, err, want_index=True, stream=None):
    """ifa_sample_verify_rows on torch cuda tensors: counts int32 [rows], ids int32 / vals int16 F16 bits [rows][k], params uint8 bytes
    of ONE sample_params_array row, draft int32 [rows - 1] (None for one row), rng_state int64 [1] (advances in place), err int32 [1].
    Returns (tokens int32 [rows], index int32 [rows] or None, n_out int32 [1]); enqueue-only."""
    import torch
    rows, k = ids.shape
    tokens = torch.empty(rows, dtype=torch.int32, device=ids.device)
    index = torch.empty(rows, dtype=torch.int32, device=ids.device) if want_index else None
    n_out = torch.empty(1, dtype=torch.int32, device=ids.device)
    check(lib().ifa_sample_verify_rows(_ptr(counts), _ptr(ids), _ptr(vals), rows, int(k), _ptr(params), _ptr(draft), _ptr(rng_state), _ptr(tokens),
                                       _ptr(index), _ptr(n_out), _ptr(err), C.c_void_p(stream)))
    return tokens, index, n_out


def logsumexp_rows(logits, n=None, row_idx=None, targets=None, split=True, stream=None):
    """ifa_logsumexp_rows over a torch cuda F16 tensor [rows_avail][stride] (or [n]): the log-sum-exp of the first n entries
    (default: all) of rows row_idx (torch cuda int32; default every row) and, with targets (torch cuda int32, one per row), the
    row's value at the target (NaN below 0).  split=False withholds the workspace (one workgroup per row).
    Returns torch cuda float32 (lse [rows], target logit [rows] or None); enqueue-only."""
    import torch
    if logits.dim() == 1:
        logits = logits.reshape(1, -1)
    stride = logits.stride(0)
    n = logits.shape[1] if n is None else int(n)
    rows = logits.shape[0] if row_idx is None else row_idx.numel()
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    tl = torch.empty(rows, dtype=torch.float32, device=logits.device) if targets is not None else None
    ws_bytes = lib().ifa_logsumexp_workspace(rows, n) if split else 0
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=logits.device) if ws_bytes else None
    check(lib().ifa_logsumexp_rows(C.c_void_p(logits.data_ptr()), stride, C.c_void_p(row_idx.data_ptr()) if row_idx is not None else None,
                                   rows, n, C.c_void_p(targets.data_ptr()) if targets is not None else None, C.c_void_p(lse.data_ptr()),
                                   C.c_void_p(tl.data_ptr()) if tl is not None else None, C.c_void_p(ws.data_ptr()) if ws is not None else None,
                                   C.c_void_p(stream)))
    lse._ifa_workspace = ws      # (alive as long as the result: the launches are only enqueued)
    return lse, tl


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def logit_adjust_rows(logits, state_slots, state, bias, params, n=None, row_idx=None, stream=None):
    """ifa_logit_adjust_rows over a torch cuda F16 tensor [rows_avail][stride] (any storage offset / stride): output row r (compact
    [rows][n] F16) = the processors of slot state_slots[r] (torch cuda int32) applied to input row row_idx[r] (torch cuda int32;
    default row r).  state: cuda int32 / uint32 bits [slots][n], bias: cuda float32 [slots][n], params: cuda float32 [slots][3]."""
    import torch
    if logits.dim() == 1:
        logits = logits.reshape(1, -1)
    n = logits.shape[1] if n is None else int(n)
    rows = state_slots.numel()
    out = torch.empty((rows, n), dtype=torch.float16, device=logits.device)
    check(lib().ifa_logit_adjust_rows(_ptr(logits), logits.stride(0), _ptr(row_idx), _ptr(state_slots), rows, n, _ptr(state), _ptr(bias), _ptr(params),
                                      _ptr(out), C.c_void_p(stream)))
    return out


def logit_adjust_draft_rows(logits, state_slot, draft, state, bias, params, n=None, stream=None):
    """ifa_logit_adjust_draft_rows over a torch cuda F16 tensor [rows][stride] (any storage offset / stride): the rows of ONE slot's
    draft step, row r adjusted as ifa_logit_adjust_rows would after ifa_logit_state_add of draft[0..r).  state_slot: cuda int32 [1];
    draft: cuda int32 [rows - 1] (None for one row); state / bias / params as in logit_adjust_rows.  Returns F16 [rows][n]."""
    import torch
    n = logits.shape[1] if n is None else int(n)
    rows = logits.shape[0]
    out = torch.empty((rows, n), dtype=torch.float16, device=logits.device)
    check(lib().ifa_logit_adjust_draft_rows(_ptr(logits), logits.stride(0), _ptr(state_slot), rows, n, _ptr(draft), _ptr(state), _ptr(bias), _ptr(params),
                                            _ptr(out), C.c_void_p(stream)))
    return out


def logit_state_reset(slot, prompt, rep, freq, pres, bias_ids, bias_vals, state, bias, params, stream=None):
    """ifa_logit_state_reset on torch cuda tensors: prompt / bias_ids int32, bias_vals float32 (None: none); state [slots][n] int32
    bits, bias [slots][n] float32, params [slots][3] float32 are updated in place; enqueue-only."""
    n_prompt = prompt.numel() if prompt is not None else 0
    n_bias = bias_ids.numel() if bias_ids is not None else 0
    check(lib().ifa_logit_state_reset(int(slot), _ptr(prompt) if n_prompt else None, n_prompt, float(rep), float(freq), float(pres),
                                      _ptr(bias_ids) if n_bias else None, _ptr(bias_vals) if n_bias else None, n_bias, state.shape[1],
                                      _ptr(state), _ptr(bias), _ptr(params), C.c_void_p(stream)))


def logit_state_add(slots, tokens, state, stream=None):
    """ifa_logit_state_add: state[slots[i]][tokens[i]] += 1 for every pair (torch cuda int32) in one launch; enqueue-only"""
    assert slots.numel() == tokens.numel()
    check(lib().ifa_logit_state_add(_ptr(slots), _ptr(tokens), slots.numel(), state.shape[1], state.shape[0], _ptr(state), C.c_void_p(stream)))


# ifa_batch_feed_row / one entry of the batched step's attention table (include/inferflow_amd.h)
BATCH_FEED_ROW = np.dtype([("live", np.int32), ("emitted", np.int32), ("kind", np.int32), ("n_stop", np.int32), ("stop_ids", np.int32, (8,)),
                           ("state_slot", np.int32), ("sel", np.int32), ("rng_final", np.uint64)])
BATCH_ATTN_ROW = np.dtype([("kc", np.uint64), ("vc", np.uint64), ("n_ctx", np.int32), ("pad", np.int32)])
BATCH_KIND_ARGMAX, BATCH_KIND_POOL_BEST, BATCH_KIND_DRAWN = 0, 1, 2
_BATCH_FEED_ARRAYS = ("rows", "step", "argmax", "pool_counts", "pool_ids", "drawn", "rng", "tok", "pos", "attn_rows", "ring", "pair_slot", "pair_tok", "err")


def _batch_feed_args(n, layers, arrays, addr):
    from ._capi import BatchFeedArgs
    unknown = set(arrays) - set(_BATCH_FEED_ARRAYS)
    assert not unknown, "batch feed: unknown arrays %s" % sorted(unknown)
    a = BatchFeedArgs()
    a.struct_size, a.n, a.layers = C.sizeof(BatchFeedArgs), int(n), int(layers)
    ring, ids = arrays["ring"], arrays.get("pool_ids")
    a.ring_steps = int(ring.shape[0])
    a.k_stride = int(ids.shape[1]) if ids is not None else 0
    for name in _BATCH_FEED_ARRAYS:
        v = arrays.get(name)
        setattr(a, name, addr(v) if v is not None else None)
    return a


def batch_feed_host(n, layers, arrays):
    """ifa_batch_feed_host (no device): one feed on numpy arrays, updated in place.  arrays: a dict by the pointer names of
    ifa_batch_feed_args -- rows BATCH_FEED_ROW [n], attn_rows BATCH_ATTN_ROW [layers][n] (None for no layers), ring int32
    [ring_steps][n], pool_ids int32 [n][k], rng uint64 [n], the others int32; argmax / pool_counts + pool_ids / drawn / rng may be
    absent.  Every array must be C-contiguous."""
    for k, v in arrays.items():
        assert v is None or (isinstance(v, np.ndarray) and v.flags.c_contiguous), k
    a = _batch_feed_args(n, layers, arrays, lambda v: v.ctypes.data)
    check(lib().ifa_batch_feed_host(C.byref(a)))


def batch_feed_rows(n, layers, arrays, stream=None):
    """ifa_batch_feed_rows: the same on torch cuda tensors (rows: the bytes of a BATCH_FEED_ROW array, attn_rows: those of a
    BATCH_ATTN_ROW array, rng int64 bits); enqueue-only."""
    for k, v in arrays.items():
        assert v is None or (v.is_cuda and v.is_contiguous()), k
    a = _batch_feed_args(n, layers, arrays, lambda v: v.data_ptr())
    check(lib().ifa_batch_feed_rows(C.byref(a), C.c_void_p(stream)))


def batch_clamp_counts(counts, pool_len, stream=None):
    """ifa_batch_clamp_counts: counts[r] = min(counts[r], pool_len[r]) in place (torch cuda int32 [rows]); enqueue-only"""
    assert counts.numel() == pool_len.numel()
    check(lib().ifa_batch_clamp_counts(_ptr(counts), _ptr(pool_len), counts.numel(), C.c_void_p(stream)))


class TpTopology(C.Structure):
    """ifa_tp_topology (include/inferflow_amd.h)"""
    _fields_ = [("tp", C.c_void_p), ("world", C.c_void_p), ("stage", C.c_int), ("n_stages", C.c_int), ("prev_rank", C.c_int),
                ("next_rank", C.c_int), ("token_src", C.c_int), ("vocab_offset", C.c_int), ("force_collectives", C.c_int)]


class Comm:
    """One rank's communicator of csrc/ifa_comm.hip (RCCL).  unique_id() on rank 0 -> ship the 128 bytes -> Comm(id, ...)."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().ifa_comm_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id, nranks, rank, device=0):
        self._h = C.c_void_p()
        self._id = C.create_string_buffer(bytes(unique_id), 128)
        check(lib().ifa_comm_init_rank(self._id, int(nranks), int(rank), int(device), C.byref(self._h)))
        self.rank, self.nranks = rank, nranks

    @classmethod
    def init_all(cls, devices):
        """One communicator per entry of `devices` in THIS process (rank threads); a device named several times makes the
        in-process loopback group (see csrc/ifa_comm.hip)."""
        n = len(devices)
        devs = (C.c_int * n)(*devices)
        hs = (C.c_void_p * n)()
        check(lib().ifa_comm_init_all(devs, n, hs))
        out = []
        for r in range(n):
            c = cls.__new__(cls)
            c._h, c._id, c.rank, c.nranks = C.c_void_p(hs[r]), None, r, n
            out.append(c)
        return out

    def all_reduce_f16(self, t, stream=None):
        check(lib().ifa_allreduce_sum_f16(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(stream)))

    def all_gather(self, src, dst, stream=None):
        check(lib().ifa_allgather(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel() * src.element_size(), C.c_void_p(stream)))

    def broadcast(self, t, root, stream=None):
        check(lib().ifa_broadcast(self._h, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), int(root), C.c_void_p(stream)))

    def send(self, t, peer, stream=None):
        check(lib().ifa_send(self._h, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), int(peer), C.c_void_p(stream)))

    def recv(self, t, peer, stream=None):
        check(lib().ifa_recv(self._h, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), int(peer), C.c_void_p(stream)))

    def oneshot(self):
        """True if small all-reduces of this communicator take the peer-mapped one-shot exchange (csrc/ifa_comm.hip)."""
        return bool(lib().ifa_comm_oneshot(self._h))

    def oneshot_export(self):
        """One process per rank: allocate this rank's one-shot buffers; returns their IPC handles (128 bytes) for the peers."""
        buf = (C.c_ubyte * 128)()
        check(lib().ifa_comm_oneshot_export(self._h, buf))
        return bytes(buf)

    def oneshot_import(self, handles_all_ranks):
        """Map the peers' buffers: handles_all_ranks = the concatenated oneshot_export() results of all ranks, in rank order."""
        b = bytes(handles_all_ranks)
        check(lib().ifa_comm_oneshot_import(self._h, (C.c_ubyte * len(b)).from_buffer_copy(b)))

    def set_oneshot(self, on):
        check(lib().ifa_comm_set_oneshot(self._h, int(bool(on))))

    def size(self):
        """Ranks of the communicator as the library reports them (ncclCommCount for RCCL communicators)."""
        return int(lib().ifa_comm_size(self._h))

    def status(self):
        return int(lib().ifa_comm_status(self._h))

    def abort(self):
        check(lib().ifa_comm_abort(self._h))

    def close(self):
        if self._h:
            lib().ifa_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tp_decode_batch(worker, tokens, positions, slots, tp=None, vocab_offset=0, logits_shard_out=None, force_collectives=False):
    """ifa_model_tp_decode_batch: one new token for each of n queries over a tensor-parallel group; returns the n tokens"""
    topo = TpTopology(tp._h if tp is not None else None, None, 0, 1, -1, -1, 0, vocab_offset, 1 if force_collectives else 0)
    toks = np.ascontiguousarray(tokens, np.int32); pos = np.ascontiguousarray(positions, np.int32); sl = np.ascontiguousarray(slots, np.int32)
    out = np.zeros(toks.size, np.int32)
    check(lib().ifa_model_tp_decode_batch(worker._h, C.byref(topo), toks.size, toks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                          sl.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                          C.c_void_p(logits_shard_out.data_ptr()) if logits_shard_out is not None else None))
    return out


def tp_prefill(worker, tokens, start_pos, tp=None, world=None, stage=0, n_stages=1, prev_rank=-1, next_rank=-1, token_src=0,
               vocab_offset=0, logits_shard_out=None, force_collectives=False):
    """ifa_model_tp_prefill: n tokens as one T > 1 step over the partition; returns the greedy next token"""
    topo = TpTopology(tp._h if tp is not None else None, world._h if world is not None else None, stage, n_stages, prev_rank,
                      next_rank, token_src, vocab_offset, 1 if force_collectives else 0)
    toks = np.ascontiguousarray(tokens, np.int32)
    nxt = C.c_int(-1)
    check(lib().ifa_model_tp_prefill(worker._h, C.byref(topo), toks.ctypes.data_as(C.c_void_p), toks.size, int(start_pos),
                                     C.c_void_p(logits_shard_out.data_ptr()) if logits_shard_out is not None else None, C.byref(nxt)))
    return nxt.value


def tp_decode(worker, first_token, start_pos, n_steps, tp=None, world=None, stage=0, n_stages=1, prev_rank=-1, next_rank=-1,
              token_src=0, vocab_offset=0, force_collectives=False):
    """ifa_model_tp_decode: the whole multi-GPU greedy decode driven from C (segments + RCCL collectives + distributed
    argmax, hipGraph per step).  Returns (tokens, gpu_ms of steps 1..n-1)."""
    topo = TpTopology(tp._h if tp is not None else None, world._h if world is not None else None, stage, n_stages, prev_rank,
                      next_rank, token_src, vocab_offset, 1 if force_collectives else 0)
    out = np.zeros(n_steps, np.int32)
    ms = C.c_float(0.0)
    check(lib().ifa_model_tp_decode(worker._h, C.byref(topo), int(first_token), int(start_pos), int(n_steps),
                                    out.ctypes.data_as(C.c_void_p), C.byref(ms)))
    return out, ms.value


def kv_shift_rows(kv_dtype, kcache_ptr, vcache_ptr, kv_heads, head_dim, rope_order, rope_cols, table_ptr, keep, discard, n_rows, stream=None):
    """ifa_kv_shift_rows: the context shift on one layer's pair of device buffers (addresses; None skips a side) with the caller's
    table of head_dim / 2 fp32 (c, s) pairs on the device.  Enqueue-only on `stream` (None: the null stream)."""
    check(lib().ifa_kv_shift_rows(int(kv_dtype), C.c_void_p(kcache_ptr), C.c_void_p(vcache_ptr), int(kv_heads), int(head_dim), int(rope_order),
                                  int(rope_cols), C.c_void_p(table_ptr), int(keep), int(discard), int(n_rows), C.c_void_p(stream)))
