"""Plain numpy / scipy statement of compare_to_baseline (compare_to_baseline.py
:36-70 the delay, :75-99 the overlap, :105-186 the metrics, :261-279 and :317-323
the texts) on arrays: in float32 as the reference runs it (numpy >= 2: the rfft
of a float32 frame is complex64, ``mc * g`` with a Python float stays float32)
and in float64 as the yardstick of the device kernels
(tests/test_gpu_compare_to_baseline.py)."""
from __future__ import annotations

import numpy as np

from tests.align_ref import FACTOR, delay_estimate, fixture, margin, power_mono  # noqa: F401

EPS = 1e-12
BANDS = [("20-80", 20, 80), ("80-200", 80, 200), ("200-1k", 200, 1000), ("1k-3k", 1000, 3000),
         ("3k-8k", 3000, 8000), ("8k-16k", 8000, 16000)]
CSV_HEADER = "freq_hz,delta_raw_db,delta_anchored_db,delta_smooth_db"


def db_bound(e32, smax, factor=FACTOR):
    """tests/compare_ref.bound moved to dB: ``factor`` times the larger of the
    float32 reference's own error and one float32 spacing at the spectrum's
    largest magnitude."""
    return factor * max(float(e32), float(np.spacing(np.float32(abs(smax)))))


def find_delay(cand, base, sr=48000, ds_sr=2000, chunk_sec=25, dtype=np.float32):
    """:36-70 -> dict(k, delay, corr, ...): layer2_analyze_eq's estimate with the
    candidate as the target (tests/align_ref.delay_estimate)."""
    return delay_estimate(cand, base, sr, ds_sr, chunk_sec, dtype)


def overlap(base, cand, delay, sr=48000, max_minutes=None):
    """:82-99 -> (base rows, cand rows)."""
    base_start, cand_start = max(0, -delay), max(0, delay)
    avail = min(len(base) - base_start, len(cand) - cand_start)
    if max_minutes is not None:
        avail = min(avail, int(max_minutes * 60 * sr))
    if avail <= 0:
        raise ValueError("no overlap after alignment")
    return base[base_start:base_start + avail], cand[cand_start:cand_start + avail]


def avg_spectrum_db(mono, n_fft, hop, dtype=np.float32):
    """:105-120 without the final cast: the float64 mean over frames of
    10 log10(|rfft(win * mono)|^2 + EPS), every frame in ``dtype``.  The window
    is the reference's float32 one in both."""
    win = np.hanning(n_fft).astype(np.float32).astype(dtype)
    mono = np.asarray(mono, dtype)
    n = len(mono)
    if n < n_fft:
        raise ValueError("segment too short")
    n_frames = 1 + (n - n_fft) // hop
    acc = np.zeros(n_fft // 2 + 1, dtype=np.float64)
    for i in range(n_frames):
        fr = mono[i * hop:i * hop + n_fft] * win
        X = np.fft.rfft(fr)
        P = (X.real * X.real + X.imag * X.imag) + EPS
        acc += 10.0 * np.log10(P)
    acc /= max(n_frames, 1)
    return acc


def smooth_1d(x, win=31):
    if win <= 1:
        return x.copy()
    w = np.ones(win, dtype=np.float32) / win
    pad = win // 2
    return np.convolve(np.pad(x, (pad, pad), mode="edge"), w, mode="valid").astype(np.float32)


def band_mean(freqs, y_db, f_lo, f_hi):
    m = (freqs >= f_lo) & (freqs < f_hi)
    if not np.any(m):
        return float("nan")
    return float(np.mean(y_db[m]))


def mono_sums(base_seg, cand_seg, g, dtype=np.float32):
    """(sum mb^2, sum mc^2, sum (mb - g mc)^2) as numpy reduces them in ``dtype``."""
    mb, mc = power_mono(base_seg, dtype), power_mono(cand_seg, dtype)
    resid = mb - (mc * g)
    return np.sum(mb * mb), np.sum(mc * mc), np.sum(resid * resid)


def compute_metrics(base_seg, cand_seg, sr=48000, n_fft=4096, hop=2048, dtype=np.float32):
    """:139-186 -> dict.  float32: the dtypes of the reference; float64: the
    power monos, every frame and the time-domain reductions in float64 (the
    spectra are cast to float32 at the end in both, as :122)."""
    mb, mc = power_mono(base_seg, dtype), power_mono(cand_seg, dtype)
    rb = np.sqrt(np.mean(mb * mb) + EPS)
    rc = np.sqrt(np.mean(mc * mc) + EPS)
    gain_db = float(20.0 * np.log10((rb + EPS) / (rc + EPS)))
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr).astype(np.float32)
    Sb64, Sc64 = avg_spectrum_db(mb, n_fft, hop, dtype), avg_spectrum_db(mc, n_fft, hop, dtype)
    Sb, Sc = Sb64.astype(np.float32), Sc64.astype(np.float32)
    delta_raw = (Sb - Sc).astype(np.float32)
    anchor = band_mean(freqs, delta_raw, 300.0, 3000.0)
    delta_anch = (delta_raw - anchor).astype(np.float32)
    delta_smooth = smooth_1d(delta_anch, win=31)
    stats = {name: band_mean(freqs, delta_smooth, lo, hi) for name, lo, hi in BANDS}
    music_err = np.nanmean([abs(stats["200-1k"]), abs(stats["1k-3k"]), abs(stats["3k-8k"])])
    noise_delta = stats["8k-16k"]
    g = 10.0 ** (gain_db / 20.0)
    resid = mb - (mc * g)
    snr = float(10.0 * np.log10((np.sum(mb * mb) + EPS) / (np.sum(resid * resid) + EPS)))
    return dict(freqs=freqs, Sb=Sb64, Sc=Sc64, delta_raw=delta_raw, delta_anch=delta_anch,
                delta_smooth=delta_smooth, gain_db=gain_db, anchor=anchor, stats=stats,
                music_err=float(music_err), noise_delta=noise_delta, snr=snr)


def run(base, cands, sr=48000, n_fft=4096, hop=2048, max_minutes=8.0, dtype=np.float32,
        delays=None):
    """The loop of main (:226-258) on arrays -> one dict per candidate (with
    ``delay``).  ``delays``: use these instead of estimating (the float64 run)."""
    out = []
    for i, cand in enumerate(cands):
        delay = find_delay(cand, base, sr)["delay"] if delays is None else delays[i]
        b, c = overlap(base, cand, delay, sr, max_minutes)
        m = compute_metrics(b, c, sr, n_fft, hop, dtype)
        m["delay"] = delay
        out.append(m)
    return out


def csv_columns(m):
    return np.column_stack([m["freqs"], m["delta_raw"], m["delta_anch"], m["delta_smooth"]])


def summary_text(baseline, paths, results, sr=48000, max_minutes=8.0):
    """summary.txt (:261-279) from ``run``'s dicts; ``paths``: the candidates'."""
    import os
    out = [f"Baseline: {baseline}\n", f"Max minutes analyzed: {max_minutes}\n", "=" * 80 + "\n\n"]
    for path, r in zip(paths, results):
        name = os.path.splitext(os.path.basename(path))[0]
        out.append(f"[{name}]\n")
        out.append(f"  file: {path}\n")
        out.append(f"  align delay (cand - base): {r['delay']} samples "
                   f"({r['delay']/sr*1000:.2f} ms)\n")
        out.append(f"  rms gain_db (base/cand): {r['gain_db']:.2f} dB\n")
        out.append(f"  anchor(300-3k) removed: {r['anchor']:.2f} dB\n")
        out.append(f"  time SNR (ref): {r['snr']:.2f} dB\n")
        out.append("  band delta (dB, baseline - candidate, anchored+smooth):\n")
        for k, _, _ in BANDS:
            out.append(f"    {k:>7}: {r['stats'][k]:+6.2f}\n")
        out.append(f"  music_err (200-8k abs avg): {r['music_err']:.2f} dB  (越小越像)\n")
        out.append(f"  noise_delta (8k-16k): {r['noise_delta']:+.2f} dB  (越接近0越像录音噪声)\n")
        out.append("\n")
    return "".join(out)


def stdout_text(outdir, paths):
    """The closing prints (:317-323)."""
    import os
    out = ["Done.", f"Outputs in: {outdir}", "  - summary.txt", "  - delta_overlay.png",
           "  - env_rms_dbfs.png"]
    out += [f"  - diff_{os.path.splitext(os.path.basename(p))[0]}.csv" for p in paths]
    return "\n".join(out) + "\n"
