"""Align, level-match and compare two renderings — MI355X drop-in for
src/compare_audio.py (workflow step 7, first half).  It
writes the ``diff_spectrum.csv`` that layer2b_apply_residual_eq[_safe] reads.

Same function names, asserts, prints and CSV as the reference; the per-sample
work runs in ``libtomatis_hip.so``:

  reference (file:line)             here
  --------------------------------- ---------------------------------------------
  find_delay_by_corr :30-42         align.find_delay_full (tm_align.hip envelope,
                                    tm_fftcorr.hip FFT correlation, arg-max)
  align_pair :44-51                 two offsets into the resident tensors
  power_mono + stft_mag_avg         analysis.stft_mag_avg(premix="power_mono",
  :61-62, :68-74, :82-86            scale=gain) (tm_analysis.hip)
  residual, rms_db :96-98           tomatis_compare_residual (two float64 means)
  band_energy, gain, diff_db,       host: the reference's numpy on n_fft / 2 + 1
  band statistics :76-80, :87-93    bins

Both files are uploaded once; the read-backs are the arg-max index, the three
mean spectra and the two residual means.

One difference in precision.  With numpy >= 2 the reference's ``c_lr2 *
gain_lin`` multiplies a float32 array by an ``np.float64`` scalar, so its
scaled candidate, that candidate's power mono, the third spectrum and the
residual are float64.  The device stays in float32 (the gain is rounded to
float32 and applied as ``scale``); the result agrees within the tolerance of
the float32 spectra (tests/test_gpu_compare.py), not bit for bit.

``compare()`` is ``main()`` minus the files.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import align, analysis, audio_io
from ._lib import RESIDUAL_DOUBLES, check, lib, ptr, stream_handle

EPS = 1e-12
BANDS = [(200, 1000), (1000, 3000), (3000, 8000), (8000, 16000)]


def power_mono(x_lr):
    """compare_audio.py:7-10 (host, elementwise)."""
    p = 0.5 * (x_lr[:, 0] ** 2 + x_lr[:, 1] ** 2)
    return np.sqrt(p + EPS)


def stft_mag_avg(x, sr, n_fft=4096, hop=2048, **kw):
    """compare_audio.py:12-24 (device)."""
    return analysis.stft_mag_avg(x, sr, n_fft, hop, **kw)


def band_energy(mag, freqs, f1, f2):
    """compare_audio.py:26-28 (host)."""
    m = (freqs >= f1) & (freqs < f2)
    return float(np.mean(mag[m] ** 2) + EPS)


def find_delay_by_corr(base, cand, sr, ds_sr=2000):
    """compare_audio.py:30-42.  ``base`` / ``cand`` are the stereo ``[n, 2]``
    signals (arrays, cuda tensors or paths): the device forms their power mono
    itself.  The reference's 1-D power-mono vectors are taken too: they go to
    the device as they are (``align.delay_full_mono``; its scipy body on the
    host for a ratio the rational decimator does not take)."""
    if not isinstance(base, str) and getattr(base, "ndim", 0) == 1:
        return align.delay_full_mono(base, cand, sr, ds_sr)
    return align.find_delay_full(base, cand, sr=sr, ds_sr=ds_sr)


def align_offsets(nb, nc, delay):
    """align_pair (:44-51) as (base start, cand start, length)."""
    b0 = -delay if delay < 0 else 0
    c0 = delay if delay > 0 else 0
    return b0, c0, max(0, min(nb - b0, nc - c0))


def align_pair(base_lr, cand_lr, delay):
    """compare_audio.py:44-51; arrays or resident tensors (row slices, no copy)."""
    b0, c0, n = align_offsets(len(base_lr), len(cand_lr), delay)
    return base_lr[b0:b0 + n], cand_lr[c0:c0 + n]


def rms_db(x):
    """compare_audio.py:53-54 (host)."""
    return 20 * np.log10(np.sqrt(np.mean(x * x) + EPS) + EPS)


def _rms_db_of_mean(m):
    return 20 * np.log10(np.sqrt(m + EPS) + EPS)


def residual_means(b_lr, c_lr, gain):
    """(mean(power_mono(b)^2), mean(power_mono(b - gain c)^2)) of two resident
    stereo tensors of equal length (:96-98)."""
    import torch
    n = b_lr.shape[0]
    assert c_lr.shape[0] == n and n >= 1
    out = torch.empty(RESIDUAL_DOUBLES, dtype=torch.float64, device="cuda")
    check(lib().tomatis_compare_residual(ptr(b_lr), ptr(c_lr), n, C.c_float(gain), ptr(out),
                                         stream_handle()), "compare_residual")
    m = out[:2].cpu().numpy()
    return float(m[0]), float(m[1])


def compare(base, cand, sr=48000, n_fft=4096, hop=2048, log=print):
    """main() of the reference minus the CSV (:57-99): returns (freqs, diff_db,
    delay, gain_db, snr_db)."""
    b_lr, sr1 = audio_io.read(base) if isinstance(base, str) else (base, sr)
    c_lr, sr2 = audio_io.read(cand) if isinstance(cand, str) else (cand, sr)
    assert sr1 == sr2 == sr and b_lr.shape[1] == 2 and c_lr.shape[1] == 2
    bd, cd = align._stereo_dev(b_lr), align._stereo_dev(c_lr)

    delay = align.find_delay_full(bd, cd, sr=sr)
    log(f"[ALIGN] delay_samples (cand - base) = {delay} ({delay/sr*1000:.2f} ms)")
    b2, c2 = align_pair(bd, cd, delay)

    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    spec = dict(premix="power_mono", as_tensor=True)
    b_mag = stft_mag_avg(b2, sr, n_fft, hop, **spec).cpu().numpy()
    c_mag = stft_mag_avg(c2, sr, n_fft, hop, **spec).cpu().numpy()
    Eb = band_energy(b_mag, freqs, 300, 3000)
    Ec = band_energy(c_mag, freqs, 300, 3000)
    gain_lin = np.sqrt(Eb / Ec)
    gain_db = 20 * np.log10(gain_lin + EPS)
    log(f"[LEVEL] anchor gain to apply on cand = {gain_db:.2f} dB (multiply by {gain_lin:.4f})")

    c_mag2 = stft_mag_avg(c2, sr, n_fft, hop, scale=float(gain_lin), **spec).cpu().numpy()
    diff_db = 20 * np.log10((b_mag + EPS) / (c_mag2 + EPS))
    for f1, f2 in BANDS:
        m = (freqs >= f1) & (freqs < f2)
        log(f"[BAND {f1}-{f2}Hz] mean ΔdB (base-cand) = {diff_db[m].mean():.2f} dB, "
            f"std={diff_db[m].std():.2f}")

    mb, mr = residual_means(b2, c2, float(gain_lin))
    snr = _rms_db_of_mean(mb) - _rms_db_of_mean(mr)
    log(f"[RESIDUAL] SNR (base vs residual) ≈ {snr:.2f} dB  (越大越像)")
    return freqs, diff_db, delay, float(gain_db), float(snr)


def main(base_path, cand_path, sr=48000, n_fft=4096, hop=2048, out_csv="diff_spectrum.csv"):
    """compare_audio.py:56-104."""
    freqs, diff_db, _, _, _ = compare(base_path, cand_path, sr, n_fft, hop)
    out = np.stack([freqs, diff_db], axis=1)
    np.savetxt(out_csv, out, delimiter=",", header="freq_hz,delta_db_base_minus_cand",
               comments="")
    print("[OUT] wrote diff_spectrum.csv")


def build_parser():
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("base", help="Base audio file")
    parser.add_argument("cand", help="Candidate audio file")
    return parser


def _cli(argv=None):
    args = build_parser().parse_args(argv)
    main(args.base, args.cand)


if __name__ == "__main__":
    _cli()


__all__ = ["power_mono", "stft_mag_avg", "band_energy", "find_delay_by_corr", "align_pair",
           "align_offsets", "rms_db", "residual_means", "compare", "main"]
