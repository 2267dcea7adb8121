"""The feed rule of a device-fed batched step (csrc/ifa_batch_feed.h) in a few lines of numpy, and the cases the CPU and the GPU
test run it on: a case is the state in front of the first feed plus what every step's kernels would have written (greedy ids,
pools, drawn ids, generator words)."""
import numpy as np

from inferflow_amd import worker as W

ARGMAX, POOL_BEST, DRAWN = W.BATCH_KIND_ARGMAX, W.BATCH_KIND_POOL_BEST, W.BATCH_KIND_DRAWN
STEP_INPUTS = ("argmax", "pool_counts", "pool_ids", "drawn", "rng")
K = 4


def feed_ref(n, layers, A):
    """one feed on the arrays of A (in place): the specification of include/inferflow_amd.h, row by row"""
    s, rows, ring = int(A["step"][0]), A["rows"], A["ring"]
    if not 0 <= s < ring.shape[0]:
        if A["err"][0] == 0:
            A["err"][0] = -1
        return
    for r in range(n):
        row = rows[r]
        if not row["live"]:
            ring[s, r] = -1
            A["pair_slot"][r] = -1
            continue
        t, j = -1, int(row["sel"])
        pooled = 0 <= j < n
        if row["kind"] == ARGMAX and A.get("argmax") is not None:
            t = int(A["argmax"][r])
        elif row["kind"] == POOL_BEST and pooled and A.get("pool_ids") is not None and A["pool_counts"][j] > 0:
            t = int(A["pool_ids"][j, 0])
        elif row["kind"] == DRAWN and pooled and A.get("drawn") is not None:
            t = int(A["drawn"][j])
        if t < 0:
            if A["err"][0] == 0:
                A["err"][0] = 1 + s * n + r
            row["live"] = 0
            ring[s, r] = -1
            A["pair_slot"][r] = -1
            continue
        ring[s, r] = t
        row["emitted"] += 1
        if A.get("rng") is not None and pooled:
            row["rng_final"] = A["rng"][j]
        A["pair_slot"][r] = row["state_slot"]
        A["pair_tok"][r] = t
        if t in [int(x) for x in row["stop_ids"][:row["n_stop"]]]:
            row["live"] = 0
            continue
        A["tok"][r] = t
        A["pos"][r] += 1
        if layers:
            A["attn_rows"]["n_ctx"][:, r] += 1
    A["step"][0] = s + 1


def fresh(n, layers, ring_steps, seed, kinds=None, with_inputs=STEP_INPUTS):
    """the state in front of step 0: every row live, kinds cycling, ragged positions, no stop ids, distinguishable filler in every
    array the feed writes"""
    g = np.random.RandomState(seed)
    rows = np.zeros(n, W.BATCH_FEED_ROW)
    rows["live"] = 1
    rows["kind"] = [(r % 3) if kinds is None else kinds[r % len(kinds)] for r in range(n)]
    rows["state_slot"] = [r if r % 2 else -1 for r in range(n)]
    # the step pools only the rows that are not plain greedy: their places among those, in row order; -1 for the others
    pooled = np.cumsum(rows["kind"] != ARGMAX) - 1
    rows["sel"] = np.where(rows["kind"] != ARGMAX, pooled, -1)
    rows["rng_final"] = g.randint(1, 1 << 48, n, dtype=np.int64).astype(np.uint64)
    pos = g.randint(0, 40, n).astype(np.int32)
    A = {"rows": rows, "step": np.zeros(1, np.int32), "tok": g.randint(3, 900, n).astype(np.int32), "pos": pos,
         "ring": np.full((ring_steps, n), -7, np.int32), "pair_slot": np.full(n, -7, np.int32), "pair_tok": np.full(n, -7, np.int32),
         "err": np.zeros(1, np.int32), "attn_rows": None}
    if layers:
        t = np.zeros((layers, n), W.BATCH_ATTN_ROW)
        t["kc"] = g.randint(1, 1 << 40, (layers, n), dtype=np.int64).astype(np.uint64)
        t["vc"] = g.randint(1, 1 << 40, (layers, n), dtype=np.int64).astype(np.uint64)
        t["n_ctx"] = pos[None, :] + 1
        t["pad"] = 0
        A["attn_rows"] = t
    shapes = {"argmax": (n,), "pool_counts": (n,), "pool_ids": (n, K), "drawn": (n,), "rng": (n,)}
    for name in with_inputs:
        A[name] = np.zeros(shapes[name], np.uint64 if name == "rng" else np.int32)
    return A


def step_inputs(n, steps, seed):
    """what the kernels in front of the feed leave per step: distinct ids per source, so that a row fed from the wrong one shows"""
    g = np.random.RandomState(seed)
    out = []
    for s in range(steps):
        out.append({"argmax": g.randint(1000, 2000, n).astype(np.int32), "pool_counts": g.randint(1, K + 1, n).astype(np.int32),
                    "pool_ids": g.randint(2000, 3000, (n, K)).astype(np.int32), "drawn": g.randint(3000, 4000, n).astype(np.int32),
                    "rng": g.randint(1, 1 << 48, n, dtype=np.int64).astype(np.uint64)})
    return out


def token_of(rows, inp, r):
    """the token row r takes from the step inputs `inp` (rows: the BATCH_FEED_ROW array with the row's kind and pool place)"""
    k, j = int(rows["kind"][r]), int(rows["sel"][r])
    return int(inp["argmax"][r]) if k == ARGMAX else int(inp["pool_ids"][j, 0]) if k == POOL_BEST else int(inp["drawn"][j])


def set_stops(A, r, ids):
    A["rows"]["n_stop"][r] = len(ids)
    A["rows"]["stop_ids"][r, :len(ids)] = ids


def cases():
    """(name, n, layers, state, [inputs of step 0, 1, ...])"""
    out = []
    # the large one: 32 rows x 80 layers, 6 steps, one row per edge of the rule
    n, layers, steps = 32, 80, 6
    A, inp = fresh(n, layers, steps, 1), step_inputs(n, steps, 2)
    rows = A["rows"]
    set_stops(A, 0, [token_of(rows, inp[0], 0)])                                              # ARGMAX, stops at step 0
    set_stops(A, 1, [5, token_of(rows, inp[2], 1)])                                           # POOL_BEST, in the middle
    set_stops(A, 2, [token_of(rows, inp[steps - 1], 2)])                                      # DRAWN, on the last step
    set_stops(A, 3, [11, 12, 13, 14, 15, 16, 17, token_of(rows, inp[3], 3)])                  # 8 stop ids, the last one hits
    set_stops(A, 4, [21, 22, 23, 24, 25, 26, 27, 28])                                         # 8 stop ids, none hits
    set_stops(A, 10, [token_of(rows, inp[1], 11), token_of(rows, inp[1], 9)])                 # only OTHER rows' tokens: never hit
    rows["n_stop"][12] = 1                                                                    # entries behind n_stop are not stop ids
    rows["stop_ids"][12] = [9, token_of(rows, inp[1], 12), 0, 0, 0, 0, 0, 0]
    rows["live"][6] = 0                                                                       # frozen before the call
    rows["emitted"][6] = 5
    inp[1]["drawn"][rows["sel"][8]] = -1                                                      # DRAWN (8 % 3 == 2): undrawable at step 1 ...
    inp[1]["pool_counts"][rows["sel"][13]] = 0                                                # ... and a POOL_BEST row too: row 8 owns the word
    inp[3]["drawn"][rows["sel"][20]] = -1                                                     # a later failure never overwrites it
    out.append(("rows32_layers80", n, layers, A, inp))
    # n = 1: one greedy row that stops on its last step
    A, inp = fresh(1, 1, 3, 3, kinds=[ARGMAX]), step_inputs(1, 3, 4)
    set_stops(A, 0, [int(inp[2]["argmax"][0])])
    out.append(("rows1_layers1", 1, 1, A, inp))
    # n = 2: a drawn row that stops in the middle next to a processed greedy row that runs on
    A, inp = fresh(2, 1, 4, 5, kinds=[DRAWN, POOL_BEST]), step_inputs(2, 4, 6)
    set_stops(A, 0, [token_of(A["rows"], inp[1], 0)])
    out.append(("rows2_layers1", 2, 1, A, inp))
    # every row stops at step 0: the steps behind it change nothing but the ring
    A, inp = fresh(3, 2, 3, 7), step_inputs(3, 3, 8)
    for r in range(3):
        set_stops(A, r, [token_of(A["rows"], inp[0], r)])
    out.append(("all_stop_at_step0", 3, 2, A, inp))
    # only the greedy ids are there: a row of another kind has no source and fails; an error word that is set is kept
    A, inp = fresh(3, 1, 3, 9, with_inputs=("argmax",)), step_inputs(3, 3, 10)
    A["err"][0] = 77
    out.append(("argmax_only_err_kept", 3, 1, A, [{"argmax": i["argmax"]} for i in inp]))
    # a step counter outside the ring: nothing changes, the error word says -1
    A, inp = fresh(2, 1, 2, 11), step_inputs(2, 3, 12)
    A["step"][0] = 2
    out.append(("step_outside_ring", 2, 1, A, inp))
    # pool places in another order than the rows, one outside 0 .. n-1, one -1: the last two rows have no pool and fail
    A, inp = fresh(4, 2, 3, 15, kinds=[DRAWN, POOL_BEST]), step_inputs(4, 3, 16)
    A["rows"]["sel"] = [2, 0, 4, -1]
    out.append(("pool_places", 4, 2, A, inp))
    # no attention table at all
    A, inp = fresh(2, 0, 3, 13, kinds=[ARGMAX]), step_inputs(2, 3, 14)
    out.append(("no_layers", 2, 0, A, inp))
    return out


def load_inputs(A, inp):
    for name, v in inp.items():
        A[name][...] = v


def clone(A):
    return {k: (None if v is None else v.copy()) for k, v in A.items()}


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        if want[k] is None:
            assert got[k] is None
            continue
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differs\n got %r\nwant %r" % (what, k, got[k], want[k])
