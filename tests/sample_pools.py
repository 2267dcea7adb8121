"""Candidate pools and parameter sets shared by the tests of the draw rule (csrc/ifa_sample_rule.h): the CPU test compares
ifa_sample_pool_host with the host sampler on them, the GPU test compares the kernel with ifa_sample_pool_host on the same ones.
A pool is (name, ids int32, F16 bits uint16) in the order ifa_topk_pool writes: value descending, lower id among equals."""
import itertools

import numpy as np

from tests.pool_util import pool_ref

COUNTS = [1, 2, 16, 17, 50, 256]             # 16 / 17: std::sort's insertion / introsort threshold
TEMPERATURES = [0.0005, 0.7, 1.0, 1.5]       # 0.0005: clamped to 0.001
TOP_PS = [0.0, 0.9, 1.0]
MAX_KS = [0, 1, 8, 300]
MIN_PS = [0.0, 0.05, 1.0]
STD, GREEDY, TOP_K, TOP_P, MIN_P = 1, 2, 3, 4, 7


def _from_values(name, vals):
    """a pool whose entry i has id 3 * i + 1 (ascending, as equal values demand) and value vals[i], sorted descending first"""
    v = np.sort(np.asarray(vals, np.float16).astype(np.float32))[::-1].astype(np.float16)
    ids = (3 * np.arange(v.size) + 1).astype(np.int32)
    return name, ids, v.view(np.uint16).copy()


def tie_pools():
    """the hand-made tie patterns"""
    rng = np.random.default_rng(11)
    out = []
    for n in (17, 64, 256):
        out.append(_from_values("all_equal_%d" % n, np.full(n, 0.25)))
    for n in (17, 50, 256):
        base = np.unique(rng.normal(0, 2.0, 4 * n).astype(np.float16))[:n].astype(np.float32)      # n distinct values
        base = np.sort(base)[::-1]
        run = max(3, n // 3)
        for where, start in (("front", 0), ("middle", (n - run) // 2), ("end", n - run)):
            v = base.copy()
            v[start:start + run] = v[start]
            out.append(_from_values("run_%s_%d" % (where, n), v))
        two = np.where(np.arange(n) % 2 == 0, 1.5, -0.75)
        out.append(_from_values("two_values_%d" % n, two))
        # several short runs: every partition of the introsort meets equal keys
        v = base.copy()
        for s in range(0, n - 4, 7):
            v[s:s + 3] = v[s]
        out.append(_from_values("short_runs_%d" % n, v))
    return out


def plain_pools():
    """every count, no ties"""
    rng = np.random.default_rng(12)
    out = []
    for n in COUNTS:
        v = np.unique(rng.normal(0, 2.0, 8 * n + 8).astype(np.float16))[:n]
        out.append(_from_values("plain_%d" % n, v))
    return out


def inf_pools():
    out = []
    rng = np.random.default_rng(13)
    for n, tail in ((17, 5), (50, 20), (256, 100)):
        v = rng.normal(0, 1.0, n).astype(np.float16)
        v[:tail] = np.float16("-inf")
        out.append(_from_values("inf_tail_%d" % n, v))
    for n in (2, 17, 50):
        out.append(_from_values("all_inf_%d" % n, np.full(n, np.float16("-inf"))))
    return out


def natural_pools(k=50):
    """the pools of 200 random F16 rows of 1000 ids with std 0.06: equal values occur by themselves"""
    rng = np.random.default_rng(14)
    out = []
    for r in range(200):
        row = rng.normal(0, 0.06, 1000).astype(np.float16)
        ids, bits = pool_ref(row, k)
        out.append(("natural_%d" % r, ids, bits))
    return out


def has_ties(bits):
    v = np.asarray(bits).view(np.float16).astype(np.float32)
    return bool(np.any(v[1:] == v[:-1]))


def combos():
    """(strategy, temperature, top_p, max_k, min_p): every value of every parameter a strategy reads, crossed"""
    out = []
    for s in (STD, TOP_P):
        out += [(s, t, p, k, 0.05) for t, p, k in itertools.product(TEMPERATURES, TOP_PS, MAX_KS)]
    out += [(TOP_K, t, 0.9, k, 0.05) for t, k in itertools.product(TEMPERATURES, MAX_KS)]
    out += [(MIN_P, t, 0.9, 8, m) for t, m in itertools.product(TEMPERATURES, MIN_PS)]
    return out


def java_random_state(seed, draws=0):
    """the generator's 48-bit state after seeding and `draws` NextDouble() calls"""
    mult, mask = 0x5DEECE66D, (1 << 48) - 1
    s = (int(seed) ^ mult) & mask
    for _ in range(2 * draws):
        s = (s * mult + 0xB) & mask
    return s
