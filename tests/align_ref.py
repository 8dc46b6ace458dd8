"""Plain numpy / scipy statement of the delay estimate (layer2_analyze_eq.py:17-52)
on arrays, in float32 as the reference runs it and in float64 as the yardstick of
the device kernels (tests/test_gpu_align.py)."""
from __future__ import annotations

import os

import numpy as np
from scipy.signal import fftconvolve, firwin, resample_poly

from tests.golden_util import GOLDEN_DIR

EPS = 1e-12
FLOOR = 2.0 ** -23
FACTOR = 8   # the rule of tests/test_gpu_spectral_fidelity.py: e <= FACTOR * max(e32, FLOOR)


def bound(e32, factor=FACTOR):
    return factor * max(float(e32), FLOOR)


def fixture(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def power_mono(x_lr, dtype=np.float32):
    x = np.asarray(x_lr, dtype)
    p = 0.5 * (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    return np.sqrt(p + EPS)


def envelope(x_lr, sr=48000, ds_sr=2000, dtype=np.float32):
    """(mean-free decimated envelope, its mean) in ``dtype``: resample_poly on
    float32 input as the reference, or on float64 input."""
    m = resample_poly(power_mono(x_lr, dtype), ds_sr, sr).astype(dtype)
    mean = np.mean(m)
    return m - mean, mean


def envelope_direct(x_lr, down, dtype=np.float64):
    """The formula the device implements, term by term: y[j] = sum_m h[m]
    e[down j + (n_taps - 1) / 2 - m] with e zero outside the signal and
    h = float32(firwin(20 down + 1, 1 / down, kaiser 5))."""
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0)).astype(np.float32).astype(dtype)
    e = power_mono(x_lr, dtype)
    half = 10 * down
    full = np.convolve(e, h)                      # full[i] = sum_m h[m] e[i - m]
    n_out = -(-len(e) // down)
    idx = down * np.arange(n_out) + half
    return full[idx]


def chunk(nbase, sr, chunk_sec):
    mid = int(0.5 * nbase)
    half = int(0.5 * chunk_sec * sr)
    return max(0, mid - half), min(nbase, mid + half)


def xcorr_valid(t, b, dtype=np.float32):
    """float32: fftconvolve as the reference (it swaps the operands when t is
    the shorter one); float64: np.correlate, which does the same."""
    if dtype == np.float32:
        return fftconvolve(t, b[::-1], mode="valid")
    return np.correlate(np.asarray(t, np.float64), np.asarray(b, np.float64), mode="valid")


def delay_estimate(target, base, sr=48000, ds_sr=2000, chunk_sec=25.0, dtype=np.float32):
    """-> dict(k, delay, corr, s, e, n_ds)."""
    s, e = chunk(len(base), sr, chunk_sec)
    mb, _ = envelope(base[s:e], sr, ds_sr, dtype)
    mt, _ = envelope(target, sr, ds_sr, dtype)
    corr = xcorr_valid(mt, mb, dtype)
    k = int(np.argmax(corr))
    base_center_sec = (s + (e - s) // 2) / sr
    targ_center_sec = (k + len(mb) // 2) / ds_sr
    delay = int(round((targ_center_sec - base_center_sec) * sr))
    return dict(k=k, delay=delay, corr=corr, s=s, e=e, n_ds=len(mb))


def margin(corr):
    """(top - runner-up) / top of a correlation."""
    c = np.sort(np.asarray(corr, np.float64))
    if len(c) < 2:
        return np.inf
    return float((c[-1] - c[-2]) / c[-1])
