"""Plain numpy statement of the audio resampler (tm_resample.hip k_rs_poly):
what ``scipy.signal.resample_poly(x, up, down, axis=0)`` computes, written out
term by term per channel, its filter, and the inputs the tests share."""
from __future__ import annotations

import functools

import numpy as np
from scipy.signal import firwin, resample_poly

from tests.rational_ref import resample_direct as _direct_1d
from tests.stft_ref import white as _white


def taps(up, down):
    """resample_poly's filter for float32 input, written independently of
    ``resample.taps``: float32(firwin) over max(up, down), scaled by up in float32."""
    m = max(up, down)
    h = firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
    return h * np.float32(up)


def taps_unscaled(up, down):
    """The same design before the scaling, as float64: scipy multiplies a
    ``window`` array by up itself."""
    m = max(up, down)
    return firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32).astype(np.float64)


def resample_direct(x, up, down, h, dtype=np.float64):
    """out[j][c] = sum_i h[down j + half - up i] x[i][c], 0 <= i < n, the tap
    index inside [0, len(h)); x is [n] or [n, ch]."""
    x = np.asarray(x)
    if x.ndim == 1:
        return _direct_1d(x, up, down, h, dtype)
    return np.stack([_direct_1d(x[:, c], up, down, h, dtype) for c in range(x.shape[1])], axis=1)


def resample_scipy64(x, up, down):
    """scipy's float64 ``resample_poly`` with the float32 design as its window: the
    statement at the lengths where ``resample_direct``'s term matrix is too large
    (tests/test_resample_ref.py holds the two together to 1e-12 of the peak).
    scipy scales the window by up in float64, ``taps`` in float32: the same taps
    where up is a power of two, which holds wherever the tests use this."""
    return resample_poly(np.asarray(x, np.float64), up, down, axis=0, window=taps_unscaled(up, down))


def random_taps(seed, n_taps):
    """A filter with no symmetry: float32 draws of a standard normal."""
    return np.random.default_rng(seed).standard_normal(n_taps).astype(np.float32)


def tapless(n_out, up, down, n_taps):
    """Mask of the output frames whose phase (down j + half) mod up has no tap
    (n_taps < up): they are +0 whatever the input is."""
    half = (n_taps - 1) // 2
    return (down * np.arange(n_out, dtype=np.int64) + half) % up >= n_taps


@functools.lru_cache(maxsize=None)
def white(seed, n, ch):
    """Uniform white noise [n, ch] of peak 0.5, float32; shared: do not write to it."""
    x = _white(seed, n, ch)
    x.setflags(write=False)
    return x


def impulse(n, ch, i0, c):
    x = np.zeros((n, ch), np.float32)
    x[i0, c] = 1.0
    return x


def impulse_response(n, up, down, h, i0):
    """The output column of a unit impulse at frame i0 of an n-frame signal:
    h[down j + half - up i0] where that index is inside the filter, else +0."""
    half = (len(h) - 1) // 2
    m = down * np.arange(-(-n * up // down), dtype=np.int64) + half - up * i0
    ok = (m >= 0) & (m < len(h))
    return np.where(ok, h[np.clip(m, 0, len(h) - 1)], np.float32(0.0)).astype(np.float32)


def edge_len(T, up, down):
    """The largest n whose outputs fit one tile of T: exactly T of them for
    up < down, the last count not above T for up > down (the count then steps by
    more than one); n + 1 frames need a second tile."""
    n = T * down // up
    assert T - up // down <= -(-n * up // down) <= T < -(-(n + 1) * up // down)
    return n
