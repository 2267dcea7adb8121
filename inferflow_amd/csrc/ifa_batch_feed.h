// ifa_batch_feed.h -- the feed rule of a device-fed batched decode step, written once for the host and the device: what the
// Infer / Commit loop does between two batched steps for each of the n rows -- take the row's token, test it against the row's
// stop ids, append it to the token ring, hand the (slot, token) pair to the logit-state counter and advance token, position and
// the per-layer context of the row -- so that the next step of the same captured graph reads its tables from device memory.
//
//   s = *step
//   for r in 0 .. n-1:
//       if !live[r]:  ring[s][r] = -1; pair_slot[r] = -1                      (tok, pos, n_ctx, rng_final, emitted unchanged)
//       else:
//           j = sel[r]               (the row's place among the rows the step pools and draws; -1: none)
//           t = choice(kind[r])      ARGMAX: argmax[r]; POOL_BEST: pool_counts[j] > 0 ? pool_ids[j][0] : -1; DRAWN: drawn[j]
//           if t < 0:                 (an empty pool, a NaN: the row cannot go on)
//               if *err == 0: *err = 1 + s * n + r
//               live[r] = 0; ring[s][r] = -1; pair_slot[r] = -1
//           else:
//               ring[s][r] = t; emitted[r]++; rng_final[r] = rng[j]            (the generator as it stands behind THIS row's draw)
//               pair_slot[r] = state_slot[r]; pair_tok[r] = t                  (what ifa_logit_state_add counts; it skips slot -1)
//               if t in stop_ids[r][0 .. n_stop): live[r] = 0                  (frozen: the row keeps its token and position)
//               else: tok[r] = t; pos[r] += 1; for every layer l: attn_rows[l][r].n_ctx += 1
//   *step = s + 1
//
// A frozen row stays in the step -- n, and with it the arithmetic of every other row, does not change -- and reprocesses the same
// token at the same position.  Its later draws move rng[r] but never rng_final[r], and nothing is counted for it.
//
// bf_feed_row is the whole rule of one row except the two parts that are not the row's own: the error word (the first failing
// row in row order owns it) and the walk over the layers' attention rows, which the kernel spreads over its threads.  Both
// callers finish those from the flags it returns.
#pragma once
#include <stddef.h>
#include "../../include/inferflow_amd.h"

#if defined(__HIPCC__)
#define IFA_BF_HD __host__ __device__ __forceinline__
#else
#define IFA_BF_HD inline
#endif

namespace ifa_bf {

// one entry of the batched step's attention table (AttnRowH of csrc/ifa_engine_state.h: the layer's K and V cache of the row's
// query and the number of keys the row attends to)
struct bf_attn_row { const void *kc, *vc; int n_ctx, pad; };
static_assert(sizeof(bf_attn_row) == IFA_BATCH_ATTN_ROW_BYTES && offsetof(bf_attn_row, n_ctx) == 16, "the attention table's entry");

enum { BF_ADVANCE = 1, BF_FAIL = 2 };

// a step pools and draws only the rows that need it: j = sel[r] is the row's place among them (0 .. n-1)
IFA_BF_HD int bf_choice(const ifa_batch_feed_args &a, int kind, int r, int j)
{
    if (kind == IFA_BATCH_KIND_ARGMAX) return a.argmax ? a.argmax[r] : -1;
    if (j < 0 || j >= a.n) return -1;
    if (kind == IFA_BATCH_KIND_POOL_BEST) return a.pool_counts && a.pool_ids && a.pool_counts[j] > 0 ? a.pool_ids[(size_t)j * (size_t)a.k_stride] : -1;
    if (kind == IFA_BATCH_KIND_DRAWN) return a.drawn ? a.drawn[j] : -1;
    return -1;
}

// the step is inside the ring (every row of a step outside it is left alone and the error word says so)
IFA_BF_HD bool bf_step_ok(const ifa_batch_feed_args &a, int s) { return s >= 0 && s < a.ring_steps; }

IFA_BF_HD int bf_err_code(const ifa_batch_feed_args &a, int s, int r) { return 1 + s * a.n + r; }

// row r of step s; returns BF_ADVANCE (every layer's n_ctx of the row is due + 1), BF_FAIL (the row could not be fed) or 0
IFA_BF_HD int bf_feed_row(const ifa_batch_feed_args &a, int s, int r)
{
    ifa_batch_feed_row &row = a.rows[r];
    int *ring = a.ring + (size_t)s * (size_t)a.n;
    if (!row.live) { ring[r] = -1; a.pair_slot[r] = -1; return 0; }
    const int j = row.sel;
    const int t = bf_choice(a, row.kind, r, j);
    if (t < 0) { row.live = 0; ring[r] = -1; a.pair_slot[r] = -1; return BF_FAIL; }
    ring[r] = t;
    row.emitted = row.emitted + 1;
    if (a.rng && j >= 0 && j < a.n) row.rng_final = a.rng[j];
    a.pair_slot[r] = row.state_slot;
    a.pair_tok[r] = t;
    const int n_stop = row.n_stop < 0 ? 0 : row.n_stop > IFA_BATCH_STOP_MAX ? IFA_BATCH_STOP_MAX : row.n_stop;
    for (int i = 0; i < n_stop; i++)
        if (row.stop_ids[i] == t) { row.live = 0; return 0; }
    a.tok[r] = t;
    a.pos[r] = a.pos[r] + 1;
    return BF_ADVANCE;
}

} // namespace ifa_bf
