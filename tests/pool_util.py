"""The candidate-pool order of SortedTopK (host/sampling_strategy.cc) / ifa_topk_pool restated in NumPy, for the pool tests."""
import numpy as np


def pool_ref(row_f16, k, excluded=()):
    """The order of SortedTopK restated: higher value first, lower id among equal values (+0.0 == -0.0), NaN and the
    excluded ids never offered.  Returns (ids, F16 bits)."""
    row = np.asarray(row_f16, np.float16)
    f = row.astype(np.float32)
    ok = ~np.isnan(f)
    if len(excluded):
        ok[np.asarray(excluded, np.int64)] = False
    ids = np.nonzero(ok)[0]
    order = np.lexsort((ids, -f[ids]))          # last key first: value descending, then id ascending (-0.0 and 0.0 tie)
    ids = ids[order][:k].astype(np.int32)
    return ids, row.view(np.uint16)[ids]


def excluded_bits(n, excluded):
    """the bitmask ifa_topk_pool takes: bit id % 32 of word id // 32"""
    bits = np.zeros((n + 31) // 32, np.uint32)
    e = np.asarray(excluded, np.int64).reshape(-1)
    np.bitwise_or.at(bits, e >> 5, (np.uint32(1) << (e & 31).astype(np.uint32)))
    return bits
