"""numpy model of the context shift's arithmetic (DESIGN.md "Context shift"; csrc/ifa_kv_shift.hip), F16 and Q8_B32T2 rows.

Every fp32 operation is one numpy float32 operation, rounded on its own; halves are rounded by numpy (round to nearest even);
the Q8 row goes dequantise -> rotate -> the store quantiser of the cache (block maximum over 32 values, scale = max / 127,
code = roundf(v / scale) clamped to -128..127 and 0 where scale <= 1e-6, scale stored as a half).  The GPU tests hold the kernel to
these bytes; tests/test_context_shift_cpu.py checks the model itself against an fp64 rotation."""
import numpy as np

F16, Q8 = 1, 8
f32 = np.float32


def row_bytes(kv_dtype, kv_heads, head_dim):
    return kv_heads * head_dim * 2 if kv_dtype == F16 else kv_heads * head_dim // 32 * 34


def pairs(head_dim, rope_order, rope_cols):
    """(table column, i0, i1) of every rotated pair of one head: order 1 pairs (2 c, 2 c + 1) for every c; order 2 pairs
    (c, c + rope_cols / 2) for 2 c < rope_cols; order 0 none"""
    if rope_order == 0:
        return []
    if rope_order == 2:
        return [(c, c, c + rope_cols // 2) for c in range(head_dim // 2) if 2 * c < rope_cols]
    return [(c, 2 * c, 2 * c + 1) for c in range(head_dim // 2)]


def unit_table(head_dim, rng):
    """head_dim / 2 random points of the unit circle as fp32 (c, s) pairs"""
    a = rng.uniform(-np.pi, np.pi, head_dim // 2)
    return np.stack([np.cos(a), np.sin(a)], 1).astype(f32)


def shift_table(head_dim, rope_dims, discard, theta=10000.0):
    """(cos, -sin) of position `discard` in fp32 numpy: angle = discard * theta ^ (-2 c / rope_dims)"""
    c = np.arange(head_dim // 2)
    ang = f32(discard) * np.power(f32(theta), (f32(-2.0) / f32(rope_dims)) * c.astype(f32)).astype(f32)
    return np.stack([np.cos(ang.astype(f32)), -np.sin(ang.astype(f32))], 1).astype(f32)


def rotate_halves(h, table, head_dim, rope_order, rope_cols):
    """h: float16 [..., head_dim]; returns the rotated copy.  x0' = f16(x0 * c - x1 * s), x1' = f16(x0 * s + x1 * c), every product,
    the difference and the sum rounded to fp32 on their own"""
    out = h.copy()
    for col, i0, i1 in pairs(head_dim, rope_order, rope_cols):
        c, s = f32(table[col, 0]), f32(table[col, 1])
        x0, x1 = h[..., i0].astype(f32), h[..., i1].astype(f32)
        out[..., i0] = ((x0 * c).astype(f32) - (x1 * s).astype(f32)).astype(f32).astype(np.float16)
        out[..., i1] = ((x0 * s).astype(f32) + (x1 * c).astype(f32)).astype(f32).astype(np.float16)
    return out


def q8_dequant(blocks):
    """blocks: uint8 [..., 34] -> float16 [..., 32]: v = f16(float(scale) * float(code))"""
    scale = np.ascontiguousarray(blocks[..., :2]).view(np.float16)[..., 0].astype(f32)
    codes = np.ascontiguousarray(blocks[..., 2:]).view(np.int8).astype(f32)
    return (scale[..., None] * codes).astype(f32).astype(np.float16)


def q8_quant(v):
    """float16 [..., 32] -> uint8 [..., 34], the cache's store quantiser"""
    x = v.astype(f32)
    mx = np.max(np.abs(x), axis=-1)
    sc = (mx / f32(127)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (x / sc[..., None]).astype(f32).astype(np.float64)
    q = np.sign(q) * np.floor(np.abs(q) + 0.5)                 # roundf: halves away from zero (exact in fp64)
    q = np.where(sc[..., None] <= f32(0.000001), 0.0, q)
    q = np.clip(q, -128, 127).astype(np.int8)
    out = np.empty(v.shape[:-1] + (34,), np.uint8)
    out[..., :2] = sc.astype(np.float16)[..., None].view(np.uint8)
    out[..., 2:] = q.view(np.uint8)
    return out


def rotate_rows(rows, kv_dtype, kv_heads, head_dim, rope_order, rope_cols, table):
    """rows: uint8 [n][row_bytes] of K cache rows -> the rows rotated by the table"""
    n = rows.shape[0]
    if rope_order == 0 or n == 0:
        return rows.copy()
    if kv_dtype == F16:
        h = np.ascontiguousarray(rows).view(np.float16).reshape(n, kv_heads, head_dim)
        return rotate_halves(h, table, head_dim, rope_order, rope_cols).reshape(n, -1).view(np.uint8)
    nb = head_dim // 32
    blocks = np.ascontiguousarray(rows).reshape(n, kv_heads, nb, 34)
    h = q8_dequant(blocks).reshape(n, kv_heads, head_dim)
    r = rotate_halves(h, table, head_dim, rope_order, rope_cols).reshape(n, kv_heads, nb, 32)
    out = q8_quant(r)
    for b in range(nb):          # a block none of whose columns is rotated keeps its bytes (requantising is not idempotent)
        if rope_order == 2 and b * 32 >= rope_cols:
            out[:, :, b] = blocks[:, :, b]
    return out.reshape(n, -1)


def shift(kbuf, vbuf, kv_dtype, kv_heads, head_dim, rope_order, rope_cols, table, keep, discard, n_rows):
    """(K bytes, V bytes) after the shift of whole cache buffers (uint8, flat); either may be None"""
    rb = row_bytes(kv_dtype, kv_heads, head_dim)
    a, b, e = keep * rb, (keep + discard) * rb, n_rows * rb
    k2 = v2 = None
    if vbuf is not None:
        v2 = vbuf.copy()
        v2[a:a + (e - b)] = vbuf[b:e]
    if kbuf is not None:
        k2 = kbuf.copy()
        moved = rotate_rows(kbuf[b:e].reshape(-1, rb), kv_dtype, kv_heads, head_dim, rope_order, rope_cols, table)
        k2[a:a + (e - b)] = moved.reshape(-1)
    return k2, v2
