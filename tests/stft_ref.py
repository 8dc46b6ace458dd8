"""A plain float64 statement of the STFT -> per-bin gain -> ISTFT -> overlap-add
operation, and the inputs, error measure and bound of the spectral-fidelity
tests (tests/test_stft_ref.py on the CPU, tests/test_gpu_spectral_fidelity.py
on the device).

``stft_ref`` takes what the C ABI takes for one stream (include/tomatis_hip.h:
TomatisStream geometry, window, gain table, one row id per frame) and loops
over frames with numpy's rfft / irfft.  ``dtype=np.float32`` runs the same
statement in float32 (numpy 2.x keeps float32 through rfft / irfft); that run
only sizes the tolerance.

Inputs are white (``white``) and the gains independent per bin
(``random_rows``), so a gain that lands on a neighbouring bin, a slip between
the two halves of the packed stereo spectrum or a slightly wrong bin moves the
output by orders of magnitude more than float32 rounding does.

Error measure for one stream (``ola_error``): compare overlap-add sums,
relative to their peak over the whole stream,

    e = max |(y - y64) * sum w^2| / max |y64 * sum w^2|

over all channels and all samples with sum w^2 >= TAU, so the 1 / sum w^2
blow-up at stream edges does not set the scale.  Bound (``bound``):
factor * max(e32, 2^-23) with e32 the float32 numpy run against float64 on the
very same case; the floor only guards against a numpy that computes in double.
"""
from __future__ import annotations

import numpy as np

TAU = 1e-3            # samples with a smaller window sum are ill-conditioned
FLOOR = 2.0 ** -23
FACTOR = 8            # device FFT: another factorisation, table twiddles, Bluestein's 3 FFTs
FACTOR_CEIL = 32      # above this a path is wrong, not imprecise
MUTATION_FACTOR = 32  # every float64 mutation of test_stft_ref.py must exceed this


def stft_ref(x, window, gains, rows, *, first_start, n_frames, hop, out_begin, out_len,
             in_scale=1.0, norm="eps", dtype=np.float64):
    """-> (y [out_len, ch], wsum [out_len], ola [out_len, ch]) in ``dtype``.

    Frame k covers input samples [first_start + k*hop, + n_fft) (zeros outside
    [0, N)), is scaled by float32 ``in_scale``, windowed, transformed, multiplied
    by ``gains[rows[k]]``, transformed back, windowed again and added at its
    position into the output range [out_begin, out_begin + out_len); ``wsum``
    adds the squared window there.  ``norm``: "eps" y = ola / (wsum + 1e-12),
    "max" y = ola / max(wsum, 1e-8)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32)
    x = x.reshape(len(x), -1)
    N, ch = x.shape
    w = np.asarray(window, np.float32).astype(dt)
    n_fft = len(w)
    g = np.asarray(gains, np.float32).astype(dt).reshape(-1, n_fft // 2 + 1)
    xs = x.astype(dt) * dt(np.float32(in_scale))
    w2 = w * w
    ola = np.zeros((out_len, ch), dt)
    wsum = np.zeros(out_len, dt)
    for k in range(n_frames):
        s = first_start + k * hop
        frame = np.zeros((n_fft, ch), dt)
        a, b = max(s, 0), min(s + n_fft, N)
        if b > a:
            frame[a - s:b - s] = xs[a:b]
        a, b = max(s, out_begin), min(s + n_fft, out_begin + out_len)
        if b <= a:
            continue
        for c in range(ch):
            X = np.fft.rfft(frame[:, c] * w) * g[int(rows[k])]
            yc = np.fft.irfft(X, n=n_fft).astype(dt) * w
            ola[a - out_begin:b - out_begin, c] += yc[a - s:b - s]
        wsum[a - out_begin:b - out_begin] += w2[a - s:b - s]
    if norm == "eps":
        den = wsum + dt(1e-12)
    elif norm == "max":
        den = np.maximum(wsum, dt(1e-8))
    else:
        raise ValueError(norm)
    return ola / den[:, None], wsum, ola


def ola_error(y, y64, wsum64, channels=None):
    """The error measure (module docstring).  ``channels``: take the numerator
    over these channels only (the scale stays the whole stream's peak)."""
    y64 = np.asarray(y64, np.float64)
    y = np.asarray(y, np.float64).reshape(y64.shape)
    m = np.asarray(wsum64, np.float64) >= TAU
    if not m.any():
        return 0.0
    ws = np.asarray(wsum64, np.float64)[m, None]
    d = np.abs((y[m] - y64[m]) * ws)
    if channels is not None:
        d = d[:, channels]
    num = float(d.max(initial=0.0))
    den = float(np.abs(y64[m] * ws).max())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def bound(e32, factor=FACTOR):
    return factor * max(float(e32), FLOOR)


def white(seed, N, ch, amp=0.5, block=0, quiet=1.0 / 32, silent=(), scaled=(), scale=1e-3):
    """Uniform white noise [N, ch] (float32) of peak ``amp``.  ``block`` > 0:
    a loud / quiet envelope shared by the channels (loud first, blocks of
    ``block`` samples, the quiet ones at ``quiet``), so that a level gate
    switches.  Channels in ``silent`` are exact zeros, those in ``scaled`` are
    multiplied by ``scale``."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (N, ch)) * amp
    if block > 0:
        x *= np.where((np.arange(N) // block) % 2 == 0, 1.0, quiet)[:, None]
    for c in scaled:
        x[:, c] *= scale
    for c in silent:
        x[:, c] = 0.0
    return x.astype(np.float32)


def random_rows(seed, n_rows, n_bins):
    """Independent uniform gains in [0.25, 1] per bin and row (float32)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.25, 1.0, (n_rows, n_bins)).astype(np.float32)


def swap_bin(g, dmin=0.1):
    """A bin k (nearest the middle of the row) with |g[k] - g[k+1]| >= dmin,
    or None."""
    g = np.asarray(g, np.float64)
    ks = np.nonzero(np.abs(np.diff(g)) >= dmin)[0]
    if len(ks) == 0:
        return None
    return int(ks[np.argmin(np.abs(ks - (len(g) - 1) // 2))])


def case_rows(seed, n_rows, n_bins):
    """``random_rows`` from the first seed in seed, seed + 1000, ... whose every
    row has a neighbouring pair of bins that differ by >= 0.1 (tiny n_bins)."""
    while True:
        g = random_rows(seed, n_rows, n_bins)
        if all(swap_bin(r) is not None for r in g):
            return g
        seed += 1000


def swapped(g, row=0):
    """(copy of the table with bins k, k+1 of ``row`` swapped, k)."""
    g = np.array(g, np.float32, copy=True).reshape(-1, np.shape(g)[-1])
    k = swap_bin(g[row])
    g[row, [k, k + 1]] = g[row, [k + 1, k]]
    return g, k


def static_geometry(N, n_fft, hop, pad):
    """Static-EQ framing (layer 2 with / without pad): frames from -n_fft/2 (or
    0) while they fit the padded stream; the output keeps the head pad."""
    pl = n_fft // 2 if pad else 0
    total = N + 2 * pl
    F = (total - n_fft) // hop + 1 if total >= n_fft else 0
    return dict(first_start=-pl, n_frames=F, hop=hop, out_begin=-pl,
                out_len=(F - 1) * hop + n_fft if F else 0)


# ---------------------------------------------------------------------------
# Shapes of the device tests (n_fft, hop): the mutation conditions of
# tests/test_stft_ref.py are checked on every one of them.
# ---------------------------------------------------------------------------

FAST_2048 = [(2048, 256), (2048, 512), (2048, 1024)]
REG_4096 = [(4096, 512), (4096, 1024), (4096, 2048)]
GENERIC_HOP = [(2048, 300), (2048, 2048), (4096, 1000)]
# any-size path in LDS: every power of two (n_fft 2 apart: its Hann window is
# all zero), hops 1, n_fft, a divisor and a non-divisor spread over the sizes
LDS_POW2 = [(4, 1), (8, 8), (16, 4), (32, 5), (64, 16), (128, 128), (256, 100),
            (512, 1), (1024, 256), (8192, 2048), (16384, 4096)]
LDS_POW2_3CH = [(2048, 512), (4096, 1000)]
# Bluestein lengths on every M = 4 ... 16384 and at its edges (2 n_fft - 1 <= M)
LDS_BLUESTEIN = [(3, 1), (5, 2), (6, 6), (9, 3), (17, 4), (31, 31), (33, 8), (100, 25),
                 (127, 50), (129, 1), (257, 64), (513, 200), (1025, 256), (1999, 500),
                 (2049, 2049), (4097, 1024), (8191, 2048)]
HBM = [(32768, 8192), (65536, 16384), (8193, 2048), (40000, 10000)]


def all_shapes():
    out = []
    for lst in (FAST_2048, REG_4096, GENERIC_HOP, LDS_POW2, LDS_POW2_3CH, LDS_BLUESTEIN, HBM):
        for s in lst:
            if s not in out:
                out.append(s)
    return out
