"""Shared by the logit-processor tests: the float32 numpy restatement of the five steps of csrc/ifa_logit_adjust.hip."""
import numpy as np

PROMPT_BIT = np.uint32(0x80000000)
F16_MAX = np.float32(65504.0)

def restate(x16, w, b, p):
    """the five steps for one row: x16 float16 [n], w uint32 [n], b float32 [n], p float32 [3] -> uint16 bits [n]"""
    rep, freq, pres = np.float32(p[0]), np.float32(p[1]), np.float32(p[2])
    with np.errstate(all="ignore"):
        x = x16.astype(np.float32)
        c = w & np.uint32(0x7FFFFFFF)
        if rep != np.float32(1.0):
            x = np.where(w != 0, np.where(x > 0, x / rep, x * rep), x).astype(np.float32)
        pen = (freq * c.astype(np.float32) + np.where(c > 0, pres, np.float32(0.0)).astype(np.float32)).astype(np.float32)
        x = (x - pen).astype(np.float32)
        x = (x + b).astype(np.float32)
        bits = np.clip(x, -F16_MAX, F16_MAX).astype(np.float16).view(np.uint16).copy()
    bits[np.isnan(x)] = 0x7E00
    bits[b == -np.inf] = 0xFC00
    return bits
