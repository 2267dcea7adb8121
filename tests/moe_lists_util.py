"""The work lists of the device-routed mixture-of-experts layer (csrc/ifa_moe.h: k_moe_build, k_moe_gather, k_moe_combine) in plain numpy, the
cases tests/test_gpu_moe_lists.py runs, the comparison it calls and the faults that comparison must reject (tests/test_moe_lists_ref_cpu.py).
No device, no library: everything here is integer bookkeeping and half arithmetic restated."""
import copy
from dataclasses import dataclass

import numpy as np

SENTINEL = 0xA5                      # every byte of an output array before the launch
GUARD = 16                           # records past an array's planned capacity that must keep it
COUNT_NAMES = ("entries", "tiles", "singles", "smalls")
KEYS = ("idx", "wdev", "epos", "tiles", "singles", "smalls", "counts")
DTYPE = dict(idx=np.int32, wdev=np.uint16, epos=np.int32, tiles=np.int32, singles=np.int32, smalls=np.int32, counts=np.int32)
WIDTH = dict(idx=1, wdev=1, epos=1, tiles=4, singles=2, smalls=4, counts=1)       # ints (halfs) per record


# ----------------------------------------------------------------------------- the reference
@dataclass
class Lists:
    idx: np.ndarray                  # int32 [entries]: token row of entry pos
    wdev: np.ndarray                 # uint16 [entries]: its weight (F16 bits)
    epos: np.ndarray                 # int32 [T * top_k]: pos of slot i, -1 none
    tiles: np.ndarray                # int32 [n][4]: expert, row0, nrows, 0
    singles: np.ndarray              # int32 [n][2]: expert, pos
    smalls: np.ndarray               # int32 [n][4]
    counts: np.ndarray               # int32 [4]: entries, tiles, singles, smalls

    def copy(self):
        return copy.deepcopy(self)


def _bits(w):
    w = np.ascontiguousarray(w)
    return (w.view(np.uint16) if w.dtype == np.float16 else w.astype(np.uint16)).reshape(-1)


def build_lists(sel, wsel, T, top_k, E, tile_rows, small_max):
    """experts ascending, token order inside an expert, the tiles of one expert in row order; slots holding -1 or any id outside [0, E) skipped"""
    sel = np.asarray(sel, np.int64).reshape(-1)
    w = _bits(wsel)
    N = T * top_k
    assert sel.size == N and w.size == N
    idx, wdev, tiles, singles, smalls = [], [], [], [], []
    epos = np.full(N, -1, np.int32)
    for e in range(E):
        slots = np.flatnonzero(sel == e)                  # ascending i = token order, then slot order
        off, c = len(idx), slots.size
        for r, i in enumerate(slots):
            idx.append(i // top_k); wdev.append(w[i]); epos[i] = off + r
        if c == 1:
            singles.append((e, off))
        elif 2 <= c <= small_max:
            smalls.append((e, off, c, 0))
        else:
            for r in range(0, c, tile_rows):
                tiles.append((e, off + r, min(tile_rows, c - r), 0))
    return Lists(np.array(idx, np.int32), np.array(wdev, np.uint16), epos, np.array(tiles, np.int32).reshape(-1, 4),
                 np.array(singles, np.int32).reshape(-1, 2), np.array(smalls, np.int32).reshape(-1, 4),
                 np.array([len(idx), len(tiles), len(singles), len(smalls)], np.int32))


def hfma(a16, w16, acc16):
    """half fma: a * w + acc rounded ONCE to half.  The product of two halfs is exact in float64; the sum is taken to 53 bits rounded to odd
    (TwoSum's remainder decides), so the final rounding to 11 bits sees what the exact sum would show it"""
    a = np.asarray(a16, np.float16).astype(np.float64)
    p = a * np.asarray(w16, np.float16).astype(np.float64)
    c = np.asarray(acc16, np.float16).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) != 0
    fix = (err != 0) & ~odd
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):                   # (past 65504: infinity, as the device rounds)
        return s.astype(np.float16)


def combine(y, epos, wsel, residual=None):
    """out[t] = residual[t] + the half fma chain over row t's slots in slot order (= ascending expert), starting from 0; the residual as ONE half
    addition behind it (float sum of the two halfs, rounded: TensorOpr::Add)"""
    y = np.asarray(y, np.float16)
    w = np.asarray(wsel)
    assert w.ndim == 2, "wsel as [T][top_k]"
    T, top_k = w.shape
    ep = np.asarray(epos, np.int64).reshape(T, top_k)
    w = w if w.dtype == np.float16 else w.astype(np.uint16).view(np.float16)
    out = np.zeros((T, y.shape[1]), np.float16)
    for j in range(top_k):
        live = ep[:, j] >= 0
        if live.any():
            out[live] = hfma(y[ep[live, j]], w[live, j][:, None], out[live])
    if residual is not None:
        with np.errstate(over="ignore"):
            out = (np.asarray(residual, np.float16).astype(np.float32) + out.astype(np.float32)).astype(np.float16)
    return out


# ----------------------------------------------------------------------------- the device's view and its comparison
def capacities(T, top_k, E, tile_rows):
    """records each output array is planned to hold (include/inferflow_amd.h: ifa_moe_build_lists)"""
    cap = T * top_k
    return dict(idx=cap, wdev=cap, epos=cap, tiles=cap // tile_rows + E, singles=E, smalls=min(E, cap // 2), counts=4)


def raw_bytes(caps, key):
    return (caps[key] + GUARD) * WIDTH[key] * np.dtype(DTYPE[key]).itemsize


def as_device(L, caps):
    """the bytes a correct launch leaves: the records, then the sentinel up to capacity + GUARD records"""
    out = {}
    for k in KEYS:
        raw = np.full(raw_bytes(caps, k), SENTINEL, np.uint8)
        rec = np.ascontiguousarray(getattr(L, k), DTYPE[k]).reshape(-1)
        assert rec.size <= caps[k] * WIDTH[k], ("the reference itself exceeds the planned capacity", k, rec.size, caps[k])
        raw[:rec.nbytes] = rec.view(np.uint8)
        out[k] = raw
    return out


def compare_lists(got, want, caps):
    """got: {name: uint8 bytes of the whole array, capacity + GUARD records}; want: Lists.  Counts first, then every list over its counted
    records bit for bit, then every byte past them up to the end of the guard"""
    counts = got["counts"][:16].view(np.int32)
    assert counts.tolist() == want.counts.tolist(), "counts %s, expected %s (%s)" % (counts.tolist(), want.counts.tolist(), ", ".join(COUNT_NAMES))
    for k in KEYS:
        rec = np.ascontiguousarray(getattr(want, k), DTYPE[k]).reshape(-1)
        g = got[k]
        assert g.size == raw_bytes(caps, k), (k, g.size)
        have = g[:rec.nbytes].view(DTYPE[k])
        if not np.array_equal(have, rec):
            at = int(np.flatnonzero(have != rec)[0])
            raise AssertionError("%s: record %d (field %d) is %d, expected %d" % (k, at // WIDTH[k], at % WIDTH[k], int(have[at]), int(rec[at])))
        rest = g[rec.nbytes:]
        assert (rest == SENTINEL).all(), "%s: byte %d past its %d records was written (capacity %d records)" % (
            k, int(np.flatnonzero(rest != SENTINEL)[0]), rec.size // WIDTH[k], caps[k])


def compare_counted(got, want, T, top_k):
    """the layer's own arrays (no sentinel behind them): got {name: array of the buffer's dtype, at least the counted records}; counts, then every
    list over its counted records, epos over all T * top_k slots"""
    counts = np.asarray(got["counts"]).reshape(-1)[:4]
    assert counts.tolist() == want.counts.tolist(), "counts %s, expected %s (%s)" % (counts.tolist(), want.counts.tolist(), ", ".join(COUNT_NAMES))
    for k in KEYS[:-1]:
        rec = np.ascontiguousarray(getattr(want, k), DTYPE[k]).reshape(-1)
        have = np.ascontiguousarray(got[k]).view(DTYPE[k]).reshape(-1)[:rec.size]
        assert rec.size == (T * top_k if k == "epos" else rec.size)
        if not np.array_equal(have, rec):
            at = int(np.flatnonzero(have != rec)[0])
            raise AssertionError("%s: record %d (field %d) is %d, expected %d" % (k, at // WIDTH[k], at % WIDTH[k], int(have[at]), int(rec[at])))


def compare_rows(got16, want16, what):
    """bit patterns of half rows (gathered rows, combined rows, sentinel rows)"""
    g, w = np.ascontiguousarray(got16).view(np.uint16), np.ascontiguousarray(want16).view(np.uint16)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d elements differ, first at %s: 0x%04x, expected 0x%04x" % (what, len(bad), bad[0].tolist(), int(g[tuple(bad[0])]),
                                                                                                int(w[tuple(bad[0])])))


# ----------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    E: int
    top_k: int
    N: int                           # T * top_k
    tile_rows: int
    small_max: int
    family: str                      # uniform | all0 | alllast | forced | forced_hi | holes
    seed: int = 0

    @property
    def T(self):
        return self.N // self.top_k

    @property
    def id(self):
        return "E%d-k%d-N%d-t%d-s%d-%s" % (self.E, self.top_k, self.N, self.tile_rows, self.small_max, self.family)


def count_edges(tile_rows, small_max):
    return [0, 1, 2, small_max, small_max + 1, tile_rows - 1, tile_rows, tile_rows + 1, 2 * tile_rows + 1]


def forced_counts(c):
    """rows per expert of a `forced` case: the count edges on neighbouring experts -- from expert 0 up (forced) or ending at expert E - 1
    (forced_hi) -- as many of them as E experts, N entries and T rows per expert allow, the large ones kept first; the other experts get 0"""
    edges = count_edges(c.tile_rows, c.small_max)
    keep = list(edges)
    while len(keep) > c.E or sum(keep) > c.N or max(keep) > c.T:
        # drop what does not fit: the largest while the sum or T is exceeded, else (too many experts) the duplicates and the middle ones
        if sum(keep) > c.N or max(keep) > c.T:
            keep.remove(max(keep))
        else:
            drop = [v for v in (c.small_max, 2, c.tile_rows - 1, 0, c.small_max + 1, 1) if v in keep]
            keep.remove(drop[0] if drop else keep[0])
    counts = [0] * c.E
    first = 0 if c.family == "forced" else c.E - len(keep)
    counts[first:first + len(keep)] = keep
    return counts


def _place(counts, T, top_k, rng):
    """sel [T][top_k] in which expert e holds counts[e] slots, no expert twice in a row; live slots first, ascending (the routers' convention)"""
    used = np.zeros(T, np.int64)
    rows = [[] for _ in range(T)]
    for e in sorted(range(len(counts)), key=lambda e: -counts[e]):
        if counts[e] == 0:
            continue
        assert counts[e] <= T
        order = np.lexsort((rng.random(T), used))          # least-filled rows first, ties at random
        for t in order[:counts[e]]:
            rows[t].append(e); used[t] += 1
    assert used.max() <= top_k, "the counts do not fit"
    sel = np.full((T, top_k), -1, np.int32)
    for t, r in enumerate(rows):
        sel[t, :len(r)] = sorted(r)
    return sel


def make_routing(c):
    """(sel int32 [T][top_k], wsel float16 [T][top_k]) of a case; the weights are all different inside a row and from the neighbouring slots"""
    rng = np.random.default_rng(1000 + 7 * c.E + 13 * c.top_k + c.N + c.tile_rows + c.small_max + len(c.family) + c.seed)
    T, K, E = c.T, c.top_k, c.E
    if c.family in ("uniform", "holes"):
        sel = np.stack([np.sort(rng.permutation(E)[:K]) for _ in range(T)]).astype(np.int32)
        if c.family == "holes":      # a third of the slots unused, anywhere in the row; some of them ids the kernel must skip, not index with
            holes = rng.random((T, K)) < 1.0 / 3.0
            junk = rng.choice(np.array([-1, -1, -1, E, 64, 1000, -7], np.int32), (T, K))
            sel = np.where(holes, junk, sel).astype(np.int32)
    elif c.family in ("all0", "alllast"):
        sel = np.full((T, K), -1, np.int32)
        sel[:, 0] = 0 if c.family == "all0" else E - 1
    elif c.family in ("forced", "forced_hi"):
        sel = _place(forced_counts(c), T, K, rng)
    else:
        raise KeyError(c.family)
    wsel = (0.05 + 0.9 * (rng.permutation(T * K).reshape(T, K) + 1) / (T * K + 1)).astype(np.float16)
    step = np.arange(T * K).reshape(T, K) % 7                # neighbouring slots never share a bit pattern
    wsel = (wsel.astype(np.float32) + step * np.float32(2.0 ** -11)).astype(np.float16)
    return sel, wsel


def _cases():
    U, A0, AL, F, FH, H = "uniform", "all0", "alllast", "forced", "forced_hi", "holes"
    rows = [
        (1, 1, 1, 64, 0, U), (1, 1, 65, 64, 8, U), (1, 1, 2400, 128, 8, U), (4, 2, 64, 64, 8, U), (4, 1, 63, 64, 0, U), (8, 8, 1024, 128, 8, U),
        (8, 2, 2400, 64, 0, U), (8, 1, 1023, 64, 8, U), (8, 1, 1025, 128, 8, U), (63, 8, 2400, 64, 8, U), (63, 1, 65, 64, 8, U), (64, 8, 64, 64, 8, U),
        (64, 2, 1024, 64, 0, U), (64, 1, 1, 64, 8, U), (64, 8, 2400, 128, 8, U),
        (4, 1, 1025, 64, 8, A0), (64, 2, 2400, 128, 8, AL), (8, 1, 64, 64, 0, AL), (63, 8, 1024, 64, 8, A0), (4, 2, 64, 64, 8, AL), (1, 1, 1024, 64, 8, A0),
        (64, 1, 1025, 64, 8, F), (64, 2, 1024, 64, 0, FH), (63, 8, 2400, 128, 8, FH), (64, 1, 1023, 64, 8, FH), (63, 2, 2400, 64, 8, F),
        (8, 2, 1024, 64, 8, F), (8, 1, 2400, 128, 8, FH), (4, 2, 64, 64, 8, F), (4, 1, 65, 64, 0, FH), (8, 8, 1024, 64, 0, F), (64, 8, 2400, 64, 0, F),
        (8, 2, 64, 64, 8, H), (64, 8, 2400, 64, 8, H), (4, 1, 1023, 64, 0, H), (63, 2, 1024, 128, 8, H), (1, 1, 63, 64, 8, H), (8, 1, 1025, 64, 8, H),
    ]
    return [Case(*r) for r in rows]


CASES = _cases()


@dataclass(frozen=True)
class RowsCase:
    """gather and combine: a routing with unused slots (entries < capacity, rows with fewer than top_k live slots, one row with none)"""
    E: int
    top_k: int
    T: int
    dim: int
    residual: bool = False

    @property
    def id(self):
        return "E%d-k%d-T%d-d%d%s" % (self.E, self.top_k, self.T, self.dim, "-res" if self.residual else "")


GATHER_CASES = [RowsCase(8, 2, 37, 256), RowsCase(8, 2, 37, 4104), RowsCase(64, 8, 5, 4104)]
COMBINE_CASES = [RowsCase(8, 2, 37, d, r) for d in (256, 250) for r in (False, True)] + [RowsCase(64, 8, 9, 250, True), RowsCase(4, 1, 3, 256, True)]


def rows_routing(c):
    rng = np.random.default_rng(50 + c.E + c.top_k + c.T)
    sel = np.stack([np.sort(rng.permutation(c.E)[:c.top_k]) for _ in range(c.T)]).astype(np.int32)
    sel = np.where(rng.random(sel.shape) < 0.3, -1, sel).astype(np.int32)
    sel[c.T // 2] = -1                                   # a row no expert takes: the combine leaves 0 (+ residual)
    if c.T > 1:
        sel[0] = np.sort(rng.permutation(c.E)[:c.top_k])  # and a full one
    wsel = rng.uniform(0.05, 0.95, sel.shape).astype(np.float16)
    return sel, wsel


def rows_data(c, n_rows, seed):
    """half rows in which every bit pattern class occurs at a known place: N(0, 1), then a few large, tiny and subnormal values"""
    rng = np.random.default_rng(seed + c.dim)
    a = rng.normal(0, 1, (n_rows, c.dim)).astype(np.float16)
    if n_rows:
        a[0, :4] = np.array([60000.0, -60000.0, 6e-8, -6.1e-5], np.float16)
        a[-1, -1] = np.float16(-0.0)
    return a


# ----------------------------------------------------------------------------- the faults
def _reorder(L, perm_of_expert_span):
    """applies a permutation to the entries [a, b) of one expert, consistently in idx, wdev and epos (a kernel filling in another order)"""
    a, b, perm = perm_of_expert_span
    R = L.copy()
    R.idx[a:b] = L.idx[a:b][perm]; R.wdev[a:b] = L.wdev[a:b][perm]
    inv = np.empty(b - a, np.int64); inv[perm] = np.arange(b - a)
    span = (L.epos >= a) & (L.epos < b)
    R.epos[span] = a + inv[L.epos[span] - a]
    return R


def _spans(L, sel, E):
    sel = np.asarray(sel).reshape(-1)
    out, off = [], 0
    for e in range(E):
        c = int((sel == e).sum())
        if c:
            out.append((e, off, off + c))
        off += c
    return out


def list_faults(L, sel, wsel, c):
    """{name: Lists} -- each a systematic mistake of k_moe_build applied to the correct lists of case c; a fault the case cannot show (no
    second tile, no single, ...) is absent"""
    sel, w = np.asarray(sel).reshape(-1), _bits(wsel)
    T, K, E = c.T, c.top_k, c.E
    out = {}
    big = [s for s in _spans(L, sel, E) if s[2] - s[1] >= 2]
    if big:
        e, a, b = big[len(big) // 2]
        out["entries of an expert in reverse order"] = _reorder(L, (a, b, np.arange(b - a)[::-1]))
        perm = np.arange(b - a); perm[[0, 1]] = [1, 0]
        out["entries of an expert in unstable order"] = _reorder(L, (a, b, perm))
    two = [i for i in range(len(L.tiles) - 1) if L.tiles[i][0] == L.tiles[i + 1][0]]
    if two:
        i = two[0]
        for name, d in (("early", -1), ("late", 1)):
            R = L.copy()
            R.tiles[i][2] += d; R.tiles[i + 1][1] += d; R.tiles[i + 1][2] -= d
            out["a tile boundary one row " + name] = R
    for name, sm in (("+ 1", c.small_max + 1), ("- 1", c.small_max - 1)):
        R = build_lists(sel, w, T, K, E, c.tile_rows, sm)
        if not (np.array_equal(R.tiles, L.tiles) and np.array_equal(R.smalls, L.smalls)):
            out["small_max treated as small_max " + name] = R
    if len(L.singles):
        R = L.copy()
        e, pos = (int(v) for v in L.singles[0])
        R.singles = L.singles[1:].copy()
        sm = [tuple(r) for r in L.smalls] + [(e, pos, 1, 0)]
        R.smalls = np.array(sorted(sm), np.int32).reshape(-1, 4)
        R.counts = np.array([L.counts[0], L.counts[1], len(R.singles), len(R.smalls)], np.int32)
        out["a single filed as a small"] = R
    ep = L.epos.reshape(T, K)
    rows2 = [(t, j) for t in range(T) for j in range(K - 1) if ep[t, j] >= 0 and ep[t, j + 1] >= 0]
    if rows2:
        t, j = rows2[len(rows2) // 2]
        R = L.copy()
        r = R.epos.reshape(T, K)
        r[t, j], r[t, j + 1] = ep[t, j + 1], ep[t, j]
        out["epos of slots j and j + 1 exchanged"] = R
    if L.counts[0]:
        live = np.flatnonzero(L.epos >= 0)
        nb = np.where(live + 1 < T * K, live + 1, live - 1)
        R = L.copy()
        R.wdev[L.epos[live]] = w[nb]
        if not np.array_equal(R.wdev, L.wdev):
            out["wdev taken from the neighbouring slot"] = R
        R = L.copy()
        R.idx[L.epos[live]] = (live % K).astype(np.int32)
        if not np.array_equal(R.idx, L.idx):
            out["idx = i % top_k in place of i / top_k"] = R
    for k, name in enumerate(COUNT_NAMES):
        for d in (1, -1):
            R = L.copy()
            R.counts[k] += d
            out["counts[%s] off by %+d" % (name, d)] = R
    return out


LIST_FAULTS = ("entries of an expert in reverse order", "entries of an expert in unstable order", "a tile boundary one row early", "a tile boundary one row late",
               "small_max treated as small_max + 1", "small_max treated as small_max - 1", "a single filed as a small", "epos of slots j and j + 1 exchanged",
               "wdev taken from the neighbouring slot", "idx = i % top_k in place of i / top_k") + tuple(
                   "counts[%s] off by %+d" % (n, d) for n in COUNT_NAMES for d in (1, -1))


def combine_faults(y, epos, wsel, residual):
    """{name: rows} -- the two mistakes a fused residual invites"""
    out = {}
    if residual is None:
        return out
    out["residual dropped"] = combine(y, epos, wsel, None)
    T, K = np.asarray(wsel).shape
    ep = np.asarray(epos, np.int64).reshape(T, K)
    acc = np.asarray(residual, np.float16).copy()
    for j in range(K):
        live = ep[:, j] >= 0
        if live.any():
            acc[live] = hfma(np.asarray(y, np.float16)[ep[live, j]], np.asarray(wsel, np.float16)[live, j][:, None], acc[live])
    out["residual added in half before, not after, the expert sum"] = acc
    return out


COMBINE_FAULTS = ("residual dropped", "residual added in half before, not after, the expert sum")
