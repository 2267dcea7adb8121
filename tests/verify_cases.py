"""Cases shared by the tests of the verify chain (csrc/ifa_sample_verify.hip): the CPU test compares ifa_sample_verify_host with a
Python chain of W.sample_pool_host on them, the GPU test compares the kernel with ifa_sample_verify_host on the same ones.
A case is `rows` pools of tests/sample_pools.py, one parameter set, a seed and the row whose draw differs from its draft."""
import numpy as np

from inferflow_amd import _capi, worker as W
from tests import sample_pools as P

MULT, MASK = 0x5DEECE66D, (1 << 48) - 1

STRATEGIES = [(P.STD, 0.7, 0.9, 8, 0.05), (P.TOP_K, 1.0, 0.9, 300, 0.05), (P.TOP_P, 1.5, 1.0, 300, 0.05), (P.MIN_P, 1.0, 0.9, 8, 0.05),
              (P.GREEDY, 1.0, 0.9, 8, 0.05)]


def advance(state, steps):
    for _ in range(steps):
        state = (state * MULT + 0xB) & MASK
    return state


def mismatch_rows(rows):
    """the acceptance outcomes of `rows` rows: the row whose draw differs from its draft -- row 0, the middle, the last draft -- and
    None: every draft accepted, `rows` tokens emitted"""
    out = [None]
    for m in (0, (rows - 1) // 2, rows - 2):
        if 0 <= m <= rows - 2 and m not in out:
            out.append(m)
    return out


def pools_of_length(n, rows, salt=0):
    """`rows` different pools of n entries: random F16 values with std 0.06 (equal values occur by themselves from ~20 entries on)"""
    rng = np.random.default_rng(1000 * n + salt)
    out = []
    for _ in range(rows):
        row = rng.normal(0, 0.06, max(4 * n, 64)).astype(np.float16)
        out.append(P.pool_ref(row, n))
    return out


def tie_pools(rows, salt=0):
    """`rows` of the hand-made tie patterns (runs of equal F16 values: the sort has something to decide), lengths 17 .. 256"""
    t = [(ids, bits) for _, ids, bits in P.tie_pools()]
    return [t[(salt + 5 * r) % len(t)] for r in range(rows)]


def arrays(pools, k_stride=None):
    rows = len(pools)
    k = k_stride or max(len(i) for i, _ in pools)
    counts = np.zeros(rows, np.int32)
    ids = np.full((rows, k), -7, np.int32)            # (slots past the count are unspecified: junk the draw must not read)
    vals = np.full((rows, k), 0x7E00, np.uint16)      # (a NaN there would fail the row if it were read)
    for r, (i, b) in enumerate(pools):
        counts[r] = len(i)
        ids[r, :len(i)] = i
        vals[r, :len(i)] = b
    return counts, ids, vals


def chain(pools, params_row, state, draft):
    """the specification in Python: W.sample_pool_host row by row, stopping at the first draw that differs from its draft or at a
    row that cannot be drawn.  Returns (tokens, index, n_out, state, err)."""
    rows = len(pools)
    toks, idxs, err = [], [], 0
    for i, (pid, bits) in enumerate(pools):
        try:
            tok, idx, _, _, _, state = W.sample_pool_host(pid, bits, params_row, state)
        except _capi.IfaError:
            err = i + 1
            break
        toks.append(tok)
        idxs.append(idx)
        if i == rows - 1 or tok != int(draft[i]):
            break
    e = len(toks)
    return (np.array(toks + [-1] * (rows - e), np.int32), np.array(idxs + [-1] * (rows - e), np.int32), e, state, err)


def drafts_for(pools, params_row, state, mismatch):
    """draft tokens under which the chain accepts rows [0, mismatch) and differs at row `mismatch` (None: accepts everything); the
    drafts behind the mismatch are junk"""
    rows = len(pools)
    draft = np.zeros(max(rows - 1, 0), np.int32)
    for i, (pid, bits) in enumerate(pools[:rows - 1]):
        tok, _, _, _, _, state = W.sample_pool_host(pid, bits, params_row, state)
        draft[i] = tok
        if mismatch is not None and i == mismatch:
            draft[i] = tok + 1
            draft[i + 1:] = 123456
            break
    return draft
