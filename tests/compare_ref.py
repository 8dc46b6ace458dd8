"""Plain numpy / scipy statement of compare_audio (compare_audio.py:30-42 and the
numbers of its main, :61-99) on arrays: in float32 as the reference runs it
(numpy >= 2: the scaled candidate is float64 from :82 on) and in float64 as
the yardstick of the device kernels (tests/test_gpu_compare.py)."""
from __future__ import annotations

import numpy as np
from scipy.signal import fftconvolve, firwin, resample_poly

from tests.align_ref import FACTOR, FLOOR, bound, fixture, margin, power_mono  # noqa: F401

EPS = 1e-12
BANDS = [(200, 1000), (1000, 3000), (3000, 8000), (8000, 16000)]


def envelope_mean_first(x_lr, sr=48000, ds_sr=2000, dtype=np.float32):
    """(resample_poly(m - m.mean(), ds_sr, sr), m.mean()) for m = power_mono (:33-34)."""
    m = power_mono(x_lr, dtype)
    mean = m.mean()
    return resample_poly(m - mean, ds_sr, sr).astype(dtype), mean


def envelope_mean_first_direct(x_lr, down, dtype=np.float64):
    """The formula the device implements: y[j] = sum_m h[m] d[down j + half - m],
    d = e - mean(e) inside the signal and zero outside it,
    h = float32(firwin(20 down + 1, 1 / down, kaiser 5))."""
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0)).astype(np.float32).astype(dtype)
    e = power_mono(x_lr, dtype)
    d = e - e.mean()
    full = np.convolve(d, h)
    idx = down * np.arange(-(-len(e) // down)) + 10 * down
    return full[idx]


def xcorr_full(c, b, dtype=np.float32):
    """float32: fftconvolve as the reference (:37); float64: np.correlate.
    out[k] = sum_j c[k - (len(b) - 1) + j] b[j]."""
    if dtype == np.float32:
        return fftconvolve(c, b[::-1], mode="full")
    return np.correlate(np.asarray(c, np.float64), np.asarray(b, np.float64), mode="full")


def delay_from_k(k, nb, sr=48000, ds_sr=2000):
    return int(round((k - (nb - 1)) * (sr / ds_sr)))


def delay_estimate(base, cand, sr=48000, ds_sr=2000, dtype=np.float32, fft64=False):
    """-> dict(k, delay, corr, nb).  fft64: the float64 correlation through
    fftconvolve (long pairs; its error is ~1e-16 of the peak)."""
    b, _ = envelope_mean_first(base, sr, ds_sr, dtype)
    c, _ = envelope_mean_first(cand, sr, ds_sr, dtype)
    corr = fftconvolve(c, b[::-1], mode="full") if fft64 else xcorr_full(c, b, dtype)
    k = int(np.argmax(corr))
    return dict(k=k, delay=delay_from_k(k, len(b), sr, ds_sr), corr=corr, nb=len(b))


def align_pair(base_lr, cand_lr, delay):
    if delay > 0:
        cand_lr = cand_lr[delay:]
    elif delay < 0:
        base_lr = base_lr[-delay:]
    n = min(len(base_lr), len(cand_lr))
    return base_lr[:n], cand_lr[:n]


def stft_mag_avg(x, n_fft, hop):
    """:12-24, frame by frame as the reference (np.hanning in float32)."""
    win = np.hanning(n_fft).astype(np.float32)
    n_frames = 1 + (len(x) - n_fft) // hop
    mags = [np.abs(np.fft.rfft(x[i * hop:i * hop + n_fft] * win)).astype(np.float32)
            for i in range(n_frames)]
    return np.stack(mags, axis=0).mean(axis=0)


def band_energy(mag, freqs, f1, f2):
    m = (freqs >= f1) & (freqs < f2)
    return float(np.mean(mag[m] ** 2) + EPS)


def rms_db(x):
    return 20 * np.log10(np.sqrt(np.mean(x * x) + EPS) + EPS)


def main_numbers(base, cand, sr=48000, n_fft=4096, hop=2048, dtype=np.float32, delay=None):
    """The numbers of main (:61-99) -> dict.  float32: the dtypes of the
    reference; float64: everything in float64."""
    b_lr, c_lr = np.asarray(base, dtype), np.asarray(cand, dtype)
    if delay is None:
        delay = delay_estimate(b_lr, c_lr, sr, 2000, dtype)["delay"]
    b_lr2, c_lr2 = align_pair(b_lr, c_lr, delay)
    b2, c2 = power_mono(b_lr2, dtype), power_mono(c_lr2, dtype)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    b_mag, c_mag = stft_mag_avg(b2, n_fft, hop), stft_mag_avg(c2, n_fft, hop)
    gain_lin = np.sqrt(band_energy(b_mag, freqs, 300, 3000) / band_energy(c_mag, freqs, 300, 3000))
    gain_db = 20 * np.log10(gain_lin + EPS)
    c_scaled = c_lr2 * gain_lin                      # float64 from here on (numpy >= 2)
    c2s = np.sqrt(0.5 * (c_scaled[:, 0] ** 2 + c_scaled[:, 1] ** 2) + EPS)
    c_mag2 = stft_mag_avg(c2s, n_fft, hop)
    diff_db = 20 * np.log10((b_mag + EPS) / (c_mag2 + EPS))
    bands = []
    for f1, f2 in BANDS:
        m = (freqs >= f1) & (freqs < f2)
        bands.append((float(diff_db[m].mean()), float(diff_db[m].std())))
    res = b_lr2 - c_scaled
    res_m = np.sqrt(0.5 * (res[:, 0] ** 2 + res[:, 1] ** 2) + EPS)
    snr = rms_db(b2) - rms_db(res_m)
    return dict(delay=delay, freqs=freqs, b_mag=b_mag, c_mag=c_mag, c_mag2=c_mag2,
                gain_lin=float(gain_lin), gain_db=float(gain_db), diff_db=diff_db, bands=bands,
                snr_db=float(snr))


def report(n, sr=48000):
    """The lines main prints from ``main_numbers``' dict."""
    out = [f"[ALIGN] delay_samples (cand - base) = {n['delay']} ({n['delay']/sr*1000:.2f} ms)",
           f"[LEVEL] anchor gain to apply on cand = {n['gain_db']:.2f} dB "
           f"(multiply by {n['gain_lin']:.4f})"]
    for (f1, f2), (mean, std) in zip(BANDS, n["bands"]):
        out.append(f"[BAND {f1}-{f2}Hz] mean ΔdB (base-cand) = {mean:.2f} dB, std={std:.2f}")
    out.append(f"[RESIDUAL] SNR (base vs residual) ≈ {n['snr_db']:.2f} dB  (越大越像)")
    out.append("[OUT] wrote diff_spectrum.csv")
    return "\n".join(out) + "\n"


def diff_db_bound(b_mag, c_mag2, mag_rtol):
    """Per-bin bound on |diff_db - golden| in dB when each mean spectrum is off
    by at most mag_rtol of its own maximum: d(20 log10 m) = (20 / ln 10) dm / m."""
    b, c = np.asarray(b_mag, np.float64), np.asarray(c_mag2, np.float64)
    return (20.0 / np.log(10.0)) * mag_rtol * (b.max() / b + c.max() / c)
