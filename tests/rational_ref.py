"""Plain numpy statement of the rational-ratio decimator (tm_align.hip
k_al_envelope): what ``scipy.signal.resample_poly(e, up, down)`` computes
for up < down, written out term by term, and the inputs of the rational delay
goldens (tests/golden/rational_cases.py), built once per process."""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.signal import firwin

from tests import align_ref as ar
from tests.golden.rational_cases import RATIONAL_CASES, make_pair


def ratio(sr, ds_sr):
    g = math.gcd(int(sr), int(ds_sr))
    return int(ds_sr) // g, int(sr) // g


def taps(up, down):
    """resample_poly's filter for float32 input, written independently of
    ``align._taps_rational``: float32(firwin) scaled by up in float32."""
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0)).astype(np.float32)
    return h * np.float32(up)


def resample_direct(e, up, down, h, dtype=np.float64):
    """out[j] = sum_i h[down j + half - up i] e[i], 0 <= i < n, the tap index
    inside [0, 2 half + 1), j < ceil(n up / down)."""
    e, h = np.asarray(e, dtype), np.asarray(h, dtype)
    n, n_taps = len(e), len(h)
    half = (n_taps - 1) // 2
    c = down * np.arange(-(-n * up // down), dtype=np.int64) + half
    t = np.arange(-(-n_taps // up), dtype=np.int64)
    m = (c % up)[:, None] + up * t[None, :]
    i = (c // up)[:, None] - t[None, :]
    ok = (m < n_taps) & (i >= 0) & (i < n)
    terms = np.where(ok, h[np.minimum(m, n_taps - 1)] * e[np.clip(i, 0, n - 1)], 0.0)
    return terms.sum(axis=1)


def outputs_per_workgroup(up, down, n_taps=None, threads=256, lds_bytes=64 * 1024):
    """T of tm_align.hip's rat_plan: the largest of 256, 128, ... 1 consecutive
    outputs whose samples, tap table and partial sums fit the LDS budget (for
    up == 1 without the table where fewer than 64 outputs fit beside it).  The
    GPU tests place their lengths on both sides of this edge."""
    n_taps = 20 * down + 1 if n_taps is None else n_taps
    K = -(-n_taps // up)
    Ks = 4 * (-(-K // 4) | 1)
    pad = 1 if up == 1 and down % 2 == 0 else 0
    for tab in [up * Ks] + ([0] if up == 1 else []):
        T = threads
        while T >= 1:
            W = (up - 1 + down * (T - 1)) // up + K
            stage = -(-(W + pad * (W // down + 1)) // 4) * 4
            if 4 * (stage + tab + threads) <= lds_bytes:
                if tab == 0 or up > 1 or T >= 64:
                    return T
                break
            T //= 2
    raise ValueError((up, down, n_taps))


def envelope_of(x, dtype=np.float32):
    """power_mono of a stereo [n, 2] signal, a 1-D vector as it is."""
    x = np.asarray(x)
    return ar.power_mono(x, dtype) if x.ndim == 2 else x.astype(dtype)


def envelope_rs(x, up, down, h, mean_first=False, dtype=np.float64):
    """(envelope as the device returns it, the mean removed) in ``dtype`` from
    the float32 signal: mean-last (layer2_analyze_eq) or mean-first (compare_audio)."""
    e = envelope_of(x, dtype)
    if mean_first:
        mean = e.mean()
        return resample_direct(e - mean, up, down, h, dtype), mean
    y = resample_direct(e, up, down, h, dtype)
    mean = y.mean()
    return y - mean, mean


@functools.lru_cache(maxsize=None)
def pair(name):
    """-> (case, target, base); arrays shared between tests: do not write to them."""
    c = next(c for c in RATIONAL_CASES if c["name"] == name)
    xt, xb = make_pair(c)
    return c, xt, xb
