"""Score N candidate renderings against one baseline — MI355X drop-in for
src/compare_to_baseline.py (workflow step 8, "产出物选择").
It writes the reference's ranked ``summary.txt``, one ``diff_<name>.csv`` per
candidate, ``delta_overlay.png`` and ``env_rms_dbfs.png``.

Same function names, arguments, defaults, error messages, CSV header, summary
text and closing prints as the reference; the per-sample work runs in
``libtomatis_hip.so``:

  reference (file:line)              here
  ---------------------------------- --------------------------------------------
  read_audio :13-15                  audio_io.read
  power_mono :17-27,                 host, a few lines (the device forms the power
  rms_dbfs_from_mono :29-31          mono inside its kernels)
  find_delay_by_corr :36-70          align.find_delay (tm_align.hip: envelope of the
                                     base's middle 25 s and of the whole candidate,
                                     valid correlation, arg-max)
  get_aligned_overlap :75-99         two offsets into the resident tensors
  avg_spectrum_db :105-122           tomatis_an_spectrum_mean (tm_analysis.hip:
                                     framing, power mono, FFT, float32 log-power,
                                     float64 sums over frames, one launch + a fold)
  rb, rc, resid, snr :144-146,       tomatis_cmp_mono_sums (tm_align.hip: three
  :182-184                           float64 sums), twice: for the gain, with it
  smooth_1d :124-131, band_mean      host: the reference's numpy on n_fft / 2 + 1
  :133-137, the rest of              values
  compute_metrics :151-178
  frame_rms_dbfs :188-202            tomatis_an_frame_r (POWER_MONO, any window
                                     length), ``20 log10(r + EPS)`` on the host
  main :207-323                      compare_many + main (argparse)

The baseline is read and uploaded once for all candidates (the reference reads
it twice per candidate) and each candidate once; the read-backs per candidate
are the arg-max, two spectra and the sums.

Precision.  The spectrum's per-frame value is float32 as the reference's (numpy
>= 2: the rfft of a float32 frame is complex64) and its sum over frames float64
as the reference's.  The time-domain means and sums are float64 sums of float32
terms where the reference reduces pairwise in float32; the results agree within
the tolerances of tests/test_gpu_compare_to_baseline.py, not bit for bit.

One deliberate narrowing: the device path is stereo only.  The reference also
takes mono files (``power_mono`` returns ``abs``); here a mono file raises a
``ValueError`` that says so.  ``avg_spectrum_db`` alone still takes a 1-D signal
as it is, like the reference's.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import align, analysis, audio_io, dsp
from ._lib import MONO_SUMS_DOUBLES, check, lib, ptr, stream_handle

EPS = 1e-12
BANDS = [("20-80", 20, 80), ("80-200", 80, 200), ("200-1k", 200, 1000), ("1k-3k", 1000, 3000),
         ("3k-8k", 3000, 8000), ("8k-16k", 8000, 16000)]
CSV_HEADER = "freq_hz,delta_raw_db,delta_anchored_db,delta_smooth_db"
STEREO_ONLY = "the device path is stereo only: audio must be [N, 2] (a mono file is not taken)"


# ---------------------------------------------------------------------------
# host functions
# ---------------------------------------------------------------------------

def read_audio(path: str):
    """compare_to_baseline.py:13-15."""
    x, sr = audio_io.read(path)
    return x, sr


def power_mono(x_lr: np.ndarray) -> np.ndarray:
    """compare_to_baseline.py:17-27 (host, elementwise)."""
    if x_lr.ndim != 2:
        raise ValueError("audio must be [N, C]")
    if x_lr.shape[1] == 1:
        return np.abs(x_lr[:, 0])
    p = 0.5 * (x_lr[:, 0] * x_lr[:, 0] + x_lr[:, 1] * x_lr[:, 1])
    return np.sqrt(p + EPS)


def rms_dbfs_from_mono(mono: np.ndarray) -> float:
    """compare_to_baseline.py:29-31 (host)."""
    r = np.sqrt(np.mean(mono * mono) + EPS)
    return float(20.0 * np.log10(r + EPS))


def smooth_1d(x: np.ndarray, win: int = 31):
    """compare_to_baseline.py:124-131 (host)."""
    if win <= 1:
        return x.copy()
    w = np.ones(win, dtype=np.float32) / win
    pad = win // 2
    xp = np.pad(x, (pad, pad), mode="edge")
    return np.convolve(xp, w, mode="valid").astype(np.float32)


def band_mean(freqs, y_db, f_lo, f_hi):
    """compare_to_baseline.py:133-137 (host)."""
    m = (freqs >= f_lo) & (freqs < f_hi)
    if not np.any(m):
        return float("nan")
    return float(np.mean(y_db[m]))


# ---------------------------------------------------------------------------
# device functions
# ---------------------------------------------------------------------------

def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _load(a, sr):
    """A path, an array or a resident tensor -> (stereo [n, 2] array or tensor,
    its sample rate: the file's, or ``sr`` for data without one)."""
    got = sr
    if isinstance(a, (str, os.PathLike)):
        a, got = read_audio(os.fspath(a))
    if not _is_tensor(a):
        a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("audio must be [N, C]")
    if a.shape[1] != 2:
        raise ValueError(STEREO_ONLY)
    return a, got


def _load_pair(base, cand, sr, message=None):
    """Both files of a comparison with the reference's rate check (before anything
    is uploaded) -> two resident float32 tensors."""
    xb, srb = _load(base, sr)
    xc, src = _load(cand, sr)
    if srb != sr or src != sr:
        raise ValueError(message or
                         f"sample rate mismatch: base={srb}, cand={src}, expected={sr}")
    return align._stereo_dev(xb), align._stereo_dev(xc)


def _resident(a, sr):
    return align._stereo_dev(_load(a, sr)[0])


def find_delay_by_corr(cand, base, sr=48000, ds_sr=2000, chunk_sec=25):
    """compare_to_baseline.py:36-70: delay = cand - base in samples (positive: the
    candidate is late).  ``cand`` / ``base``: paths, arrays or resident tensors."""
    xb, xc = _load_pair(base, cand, sr)
    return align.find_delay(xc, xb, sr=sr, ds_sr=ds_sr, chunk_sec=chunk_sec)


def _overlap(xb, xc, sr, max_minutes):
    """:81-99 on two resident tensors."""
    delay = align.find_delay(xc, xb, sr=sr)
    base_start = max(0, -delay)
    cand_start = max(0, delay)
    avail = min(xb.shape[0] - base_start, xc.shape[0] - cand_start)
    if max_minutes is not None:
        avail = min(avail, int(max_minutes * 60 * sr))
    if avail <= 0:
        raise ValueError("no overlap after alignment")
    return xb[base_start:base_start + avail], xc[cand_start:cand_start + avail], delay


def get_aligned_overlap(base, cand, sr=48000, max_minutes=None):
    """compare_to_baseline.py:75-99 -> (base rows, cand rows, delay): row slices of
    the resident tensors, no copy."""
    xb, xc = _load_pair(base, cand, sr, "sample rate mismatch")
    return _overlap(xb, xc, sr, max_minutes)


def spectrum_mean(xd, n_fft, hop, sig, ch, scale=1.0):
    """tomatis_an_spectrum_mean on a resident tensor -> float64 cuda tensor of
    n_fft / 2 + 1 means."""
    import torch
    analysis._check_n_fft(n_fft)
    n = xd.shape[0]
    F = analysis._n_frames(n, n_fft, hop)
    nb = n_fft // 2 + 1
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    work = torch.empty(int(lib().tomatis_an_spectrum_mean_work_doubles(F, nb)), dtype=torch.float64,
                       device="cuda")
    out = torch.empty(nb, dtype=torch.float64, device="cuda")
    check(lib().tomatis_an_spectrum_mean(ptr(xd), n, ch, n_fft, hop, sig, C.c_float(scale),
                                         ptr(win), ptr(work), ptr(out), stream_handle()),
          "an_spectrum_mean")
    return out


def avg_spectrum_db(x, sr: int, n_fft: int, hop: int):
    """compare_to_baseline.py:105-122 -> (freqs float32, spec float32).  ``x`` is
    the stereo ``[n, 2]`` signal whose power mono the reference would pass (formed
    on the device), or a 1-D signal taken as it is."""
    if getattr(x, "ndim", None) is None:
        x = np.asarray(x)
    if x.ndim == 2 and x.shape[1] != 2:
        raise ValueError(STEREO_ONLY)
    if x.shape[0] < n_fft:
        raise ValueError("segment too short")
    if x.ndim == 1:
        xd, sig, ch = analysis._dev(x).reshape(-1), analysis.AN_SIG_RAW, 1
    else:
        xd, sig, ch = analysis._dev(x, ch=2), analysis.AN_SIG_POWER_MONO, 2
    acc = spectrum_mean(xd, n_fft, hop, sig, ch).cpu().numpy()
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    return freqs.astype(np.float32), acc.astype(np.float32)


def mono_sums(b_lr, c_lr, gain=0.0):
    """(sum mb^2, sum mc^2, sum (mb - gain mc)^2) of two resident stereo tensors of
    equal length (:144-145, :183-184): float32 terms, float64 sums."""
    import torch
    n = b_lr.shape[0]
    if c_lr.shape[0] != n or n < 1:
        raise ValueError("mono_sums needs two segments of one length >= 1")
    out = torch.empty(MONO_SUMS_DOUBLES, dtype=torch.float64, device="cuda")
    check(lib().tomatis_cmp_mono_sums(ptr(b_lr), ptr(c_lr), n, C.c_float(gain), ptr(out),
                                      stream_handle()), "cmp_mono_sums")
    s = out[:3].cpu().numpy()
    return float(s[0]), float(s[1]), float(s[2])


def compute_metrics(base_seg, cand_seg, sr=48000, n_fft=4096, hop=2048):
    """compare_to_baseline.py:139-186 -> (freqs, delta_raw, delta_anch,
    delta_smooth, gain_db, anchor, stats, music_err, noise_delta, snr)."""
    xb, xc = _resident(base_seg, sr), _resident(cand_seg, sr)
    n = xb.shape[0]

    sb, sc, _ = mono_sums(xb, xc)
    rb = np.sqrt(sb / n + EPS)
    rc = np.sqrt(sc / n + EPS)
    gain_db = float(20.0 * np.log10((rb + EPS) / (rc + EPS)))

    freqs, Sb = avg_spectrum_db(xb, sr, n_fft, hop)
    _, Sc = avg_spectrum_db(xc, sr, n_fft, hop)
    delta_raw = (Sb - Sc).astype(np.float32)  # base - cand

    anchor = band_mean(freqs, delta_raw, 300.0, 3000.0)
    delta_anch = (delta_raw - anchor).astype(np.float32)
    delta_smooth = smooth_1d(delta_anch, win=31)

    stats = {name: band_mean(freqs, delta_smooth, lo, hi) for name, lo, hi in BANDS}
    music_err = np.nanmean([abs(stats["200-1k"]), abs(stats["1k-3k"]), abs(stats["3k-8k"])])
    noise_delta = stats["8k-16k"]

    g = 10.0 ** (gain_db / 20.0)
    sb, _, sr2 = mono_sums(xb, xc, g)
    snr = float(10.0 * np.log10((sb + EPS) / (sr2 + EPS)))
    return (freqs, delta_raw, delta_anch, delta_smooth, gain_db, anchor, stats, music_err,
            noise_delta, snr)


def frame_r(x, win, hop):
    """Per-window ``sqrt(mean(power_mono^2) + EPS)`` of a stereo signal in
    numpy's float32 pairwise order (tomatis_an_frame_r): float32 array."""
    xd = _resident(x, 0)
    r = analysis._frame_r(xd, xd.shape[0], 2, win, hop, analysis.AN_LEVEL_POWER_MONO)
    return r.cpu().numpy()


def frame_rms_dbfs(x, sr: int, win_ms=50, hop_ms=25):
    """compare_to_baseline.py:188-202 of the stereo ``x``'s power mono -> (t, y)."""
    win = int(sr * win_ms / 1000.0)
    hop = int(sr * hop_ms / 1000.0)
    win = max(win, 256)
    hop = max(hop, 128)
    n = x.shape[0]
    if n < win:
        host = x.cpu().numpy() if _is_tensor(x) else np.asarray(x)
        if host.ndim != 2 or host.shape[1] != 2:
            raise ValueError(STEREO_ONLY)
        return np.array([0.0]), np.array([rms_dbfs_from_mono(power_mono(host))])
    n_frames = 1 + (n - win) // hop
    t = (np.arange(n_frames) * hop) / sr
    y = 20.0 * np.log10(frame_r(x, win, hop) + EPS)
    return t.astype(np.float32), y.astype(np.float32)


# ---------------------------------------------------------------------------
# the multi-candidate run
# ---------------------------------------------------------------------------

def _write_summary(path, baseline, max_minutes, results, sr):
    """:261-279."""
    with open(path, "w", encoding="utf-8") as f:
        f.write(f"Baseline: {baseline}\n")
        f.write(f"Max minutes analyzed: {max_minutes}\n")
        f.write("=" * 80 + "\n\n")
        for r in results:
            f.write(f"[{r['name']}]\n")
            f.write(f"  file: {r['path']}\n")
            f.write(f"  align delay (cand - base): {r['delay']} samples "
                    f"({r['delay']/sr*1000:.2f} ms)\n")
            f.write(f"  rms gain_db (base/cand): {r['gain_db']:.2f} dB\n")
            f.write(f"  anchor(300-3k) removed: {r['anchor_db']:.2f} dB\n")
            f.write(f"  time SNR (ref): {r['snr']:.2f} dB\n")
            f.write("  band delta (dB, baseline - candidate, anchored+smooth):\n")
            for k, _, _ in BANDS:
                f.write(f"    {k:>7}: {r['stats'][k]:+6.2f}\n")
            f.write(f"  music_err (200-8k abs avg): {r['music_err']:.2f} dB  (越小越像)\n")
            f.write(f"  noise_delta (8k-16k): {r['noise_delta']:+.2f} dB  (越接近0越像录音噪声)\n")
            f.write("\n")


def _plots(outdir, results, sr):
    """:281-315: delta_overlay.png and env_rms_dbfs.png."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(12, 5))
    for r in results:
        plt.semilogx(r["freqs"], r["delta_smooth"], label=r["name"])
    plt.axhline(0.0, linewidth=1)
    plt.title("Candidate vs Baseline (Delta = base - cand, anchored@300-3k, smooth)")
    plt.xlabel("Frequency (Hz)")
    plt.ylabel("Delta dB (base - candidate)")
    plt.grid(True, which="both", ls="--", alpha=0.4)
    plt.legend()
    plt.tight_layout()
    plt.savefig(os.path.join(outdir, "delta_overlay.png"), dpi=160)
    plt.close()

    # the baseline's envelope over the first candidate's overlap, as the reference
    plt.figure(figsize=(12, 6))
    tb, eb = frame_rms_dbfs(results[0]["xb_seg"], sr)
    plt.plot(tb, eb, label="baseline")
    for r in results:
        tc, ec = frame_rms_dbfs(r["xc_seg"], sr)
        plt.plot(tc, ec, label=r["name"], alpha=0.8)
    plt.title("RMS dBFS Envelope (aligned overlap)")
    plt.xlabel("Time (s)")
    plt.ylabel("RMS dBFS")
    plt.grid(True, ls="--", alpha=0.4)
    plt.legend()
    plt.tight_layout()
    plt.savefig(os.path.join(outdir, "env_rms_dbfs.png"), dpi=160)
    plt.close()


def compare_many(baseline, candidates, outdir, sr=48000, n_fft=4096, hop=2048, max_minutes=8.0,
                 names=None):
    """main() of the reference minus argparse (:218-323); returns the results
    list.  ``baseline`` / ``candidates``: paths (or arrays / resident tensors with
    ``names`` for the CSV files and the summary)."""
    os.makedirs(outdir, exist_ok=True)
    xb = None
    results = []
    for i, cand in enumerate(candidates):
        # the baseline is uploaded once and stays resident for every candidate
        xb, xc = _load_pair(baseline if xb is None else xb, cand, sr, "sample rate mismatch")
        xb_seg, xc_seg, delay = _overlap(xb, xc, sr, max_minutes)
        (freqs, d_raw, d_anch, d_smooth, gain_db, anchor, stats, music_err, noise_delta,
         snr) = compute_metrics(xb_seg, xc_seg, sr=sr, n_fft=n_fft, hop=hop)

        if names is not None:
            name = names[i]
        else:
            name = os.path.splitext(os.path.basename(cand))[0]
        np.savetxt(os.path.join(outdir, f"diff_{name}.csv"),
                   np.column_stack([freqs, d_raw, d_anch, d_smooth]), delimiter=",",
                   header=CSV_HEADER, comments="")
        results.append({
            "name": name, "path": cand if names is None else name, "delay": delay,
            "gain_db": gain_db, "anchor_db": anchor, "snr": snr, "stats": stats,
            "music_err": music_err, "noise_delta": noise_delta, "freqs": freqs,
            "delta_raw": d_raw, "delta_anch": d_anch, "delta_smooth": d_smooth,
            "xb_seg": xb_seg, "xc_seg": xc_seg})

    _write_summary(os.path.join(outdir, "summary.txt"),
                   baseline if isinstance(baseline, (str, os.PathLike)) else "baseline",
                   max_minutes, results, sr)
    _plots(outdir, results, sr)

    print("Done.")
    print(f"Outputs in: {outdir}")
    print("  - summary.txt")
    print("  - delta_overlay.png")
    print("  - env_rms_dbfs.png")
    for r in results:
        print(f"  - diff_{r['name']}.csv")
    return results


def build_parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", required=True)
    ap.add_argument("--candidates", required=True, nargs="+")
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--n_fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=2048)
    ap.add_argument("--max_minutes", type=float, default=8.0)
    return ap


def main(argv=None):
    """compare_to_baseline.py:207-323."""
    args = build_parser().parse_args(argv)
    compare_many(args.baseline, args.candidates, args.outdir, sr=args.sr, n_fft=args.n_fft,
                 hop=args.hop, max_minutes=args.max_minutes)


if __name__ == "__main__":
    main()


__all__ = ["read_audio", "power_mono", "rms_dbfs_from_mono", "smooth_1d", "band_mean",
           "find_delay_by_corr", "get_aligned_overlap", "avg_spectrum_db", "spectrum_mean",
           "mono_sums", "compute_metrics", "frame_r", "frame_rms_dbfs", "compare_many", "main"]
