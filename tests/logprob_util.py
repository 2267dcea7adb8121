"""Shared by the log-probability tests: the float64 statement of a row's log-sum-exp and the fp32 error bound of the device
kernel's prescribed structure (csrc/ifa_logprob.hip)."""
import math

import numpy as np


def lse_f64(row_f16, n=None):
    """max + log(sum exp(x - max)) in float64 over the first n entries; NaN for a NaN or +inf entry or a row of -inf only"""
    x = np.asarray(row_f16)[:n].astype(np.float64)
    if np.isnan(x).any() or np.isposinf(x).any() or np.isneginf(x).all():
        return float("nan")
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def bound(n, lse):
    """worst-case fp32 error of the structure: chain adds (twice: an online rescale), an 11-level tree plus the cross-wave combine,
    one expf and one log, one rounding of the result"""
    return (2 * math.ceil(n / 2048) + 24) * 2.0 ** -24 + 2.0 ** -23 * max(1.0, abs(lse))


def check_lse(got, want, n, what=""):
    """got against the float64 value: NaN exactly where the definition is NaN, else inside the bound; returns |error| / bound"""
    if math.isnan(want):
        assert math.isnan(got), (what, got)
        return 0.0
    assert not math.isnan(got), (what, want)
    err = abs(float(got) - want)
    assert err <= bound(n, want), (what, n, float(got), want, err, bound(n, want))
    return err / bound(n, want)
