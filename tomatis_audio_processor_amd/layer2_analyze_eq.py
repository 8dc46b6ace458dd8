"""Static EQ curve between a baseline recording and a rendered file — MI355X
drop-in for src/layer2_analyze_eq.py (workflow step 5).

Same functions, flags, defaults, prints, errors, CSV and PNG as the reference;
the per-sample work runs in ``libtomatis_hip.so``:

  reference (file:line)            here
  -------------------------------- ----------------------------------------------
  find_delay_by_corr :17-52        align.find_delay (tm_align.hip)
  stft_logpower_median :54-88      analysis.stft_logpower_median (tm_analysis.hip)
  anchor median, clip, savgol      host: the reference's own numpy / scipy calls on
  :135-153, CSV :156-157, PNG      n_fft / 2 + 1 bins

``analyze()`` is ``main()`` minus argparse and the files.
"""
from __future__ import annotations

import argparse

import numpy as np

from . import align, analysis, audio_io

EPS = 1e-12


def power_mono(x_lr: np.ndarray) -> np.ndarray:
    """layer2_analyze_eq.py:9-11 (host, elementwise)."""
    p = 0.5 * (x_lr[:, 0] * x_lr[:, 0] + x_lr[:, 1] * x_lr[:, 1])
    return np.sqrt(p + EPS)


def rms_dbfs(mono: np.ndarray) -> float:
    """layer2_analyze_eq.py:13-15 (host)."""
    r = np.sqrt(np.mean(mono * mono) + EPS)
    return float(20.0 * np.log10(r + EPS))


def find_delay_by_corr(target_path, base_path, sr=48000, ds_sr=2000, chunk_sec=25.0):
    """layer2_analyze_eq.py:17-52: delay = target - base in samples (device)."""
    return align.find_delay(target_path, base_path, sr=sr, ds_sr=ds_sr, chunk_sec=chunk_sec)


def stft_logpower_median(x_lr, sr: int, n_fft: int, hop: int, music_dbfs: float):
    """layer2_analyze_eq.py:54-88 -> (freqs, median log-power dB, used frames) (device)."""
    return analysis.stft_logpower_median(x_lr, sr, n_fft, hop, music_dbfs)


def eq_tail(freqs, med_b, med_t, anchor_lo=300.0, anchor_hi=3000.0, clamp_db=12.0,
            smooth_bins=71):
    """layer2_analyze_eq.py:135-153 on the two medians: (delta0, delta_s, anchor)."""
    from scipy.signal import savgol_filter
    delta = (med_b - med_t).astype(np.float32)
    anchor_mask = (freqs >= anchor_lo) & (freqs <= anchor_hi)
    anchor = float(np.median(delta[anchor_mask]))
    delta0 = (delta - anchor).astype(np.float32)
    clamp = float(clamp_db)
    delta0 = np.clip(delta0, -clamp, +clamp)
    w = int(smooth_bins)
    if w % 2 == 0:
        w += 1
    w = max(11, w)
    if w >= len(delta0):
        w = len(delta0) - 1 if (len(delta0) - 1) % 2 == 1 else len(delta0) - 2
    delta_s = savgol_filter(delta0, window_length=w, polyorder=3).astype(np.float32)
    return delta0, delta_s, anchor


def analyze(base, target, sr=48000, max_minutes=6.0, n_fft=8192, hop=4096, music_dbfs=-65.0,
            anchor_lo=300.0, anchor_hi=3000.0, clamp_db=12.0, smooth_bins=71, log=print):
    """main() of the reference minus argparse, the CSV and the PNG (:107-153):
    returns (freqs, delta0, delta_s, anchor, used_b, used_t, delay)."""
    xb_all, srb = audio_io.read(base) if isinstance(base, str) else (base, sr)
    xt_all, srt = audio_io.read(target) if isinstance(target, str) else (target, sr)
    assert srb == sr and srt == sr
    assert xb_all.shape[1] == 2 and xt_all.shape[1] == 2
    delay = align.find_delay(xt_all, xb_all, sr=sr)
    log(f"[ALIGN] delay (target - base): {delay} samples ({delay/sr*1000:.2f} ms)")
    base_start = max(0, -delay)
    targ_start = max(0, delay)
    max_len = int(max_minutes * 60 * sr)
    avail = min(len(xb_all) - base_start, len(xt_all) - targ_start, max_len)
    if avail <= n_fft:
        raise ValueError("对齐后可用重叠太短，无法统计。")
    xb = xb_all[base_start:base_start + avail]
    xt = xt_all[targ_start:targ_start + avail]
    freqs, med_b, used_b = stft_logpower_median(xb, sr, n_fft, hop, music_dbfs)
    _, med_t, used_t = stft_logpower_median(xt, sr, n_fft, hop, music_dbfs)
    log(f"[STATS] used music frames (base/target): {used_b}/{used_t}")
    delta0, delta_s, anchor = eq_tail(freqs, med_b, med_t, anchor_lo, anchor_hi, clamp_db,
                                      smooth_bins)
    return freqs, delta0, delta_s, anchor, used_b, used_t, delay


def _plot(path, freqs, delta0, delta_s, sr, clamp):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(12, 6))
    plt.plot(freqs, delta0, label="raw (anchored, clamped)")
    plt.plot(freqs, delta_s, label="smooth")
    plt.xscale("log")
    plt.xlim(20, sr / 2)
    plt.ylim(-clamp - 1, clamp + 1)
    plt.grid(True, which="both", ls="--", alpha=0.4)
    plt.xlabel("Frequency (Hz)")
    plt.ylabel("Delta (dB)  [base - target]")
    plt.title("Layer2 EQ Curve (Static)")
    plt.legend()
    plt.tight_layout()
    plt.savefig(path, dpi=150)
    plt.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="基准（录音参照）")
    ap.add_argument("--target", required=True, help="要匹配的目标（D_MNF_matched_v2）")
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--max_minutes", type=float, default=6.0, help="用于统计的最长时长（分钟）")
    ap.add_argument("--n_fft", type=int, default=8192)
    ap.add_argument("--hop", type=int, default=4096)
    ap.add_argument("--music_dbfs", type=float, default=-65.0)
    ap.add_argument("--anchor_lo", type=float, default=300.0)
    ap.add_argument("--anchor_hi", type=float, default=3000.0)
    ap.add_argument("--clamp_db", type=float, default=12.0, help="限制 EQ 幅度，避免过拟合/失真")
    ap.add_argument("--smooth_bins", type=int, default=71, help="频率方向平滑窗口（奇数更好）")
    ap.add_argument("--out_csv", default="layer2_eq_curve.csv")
    ap.add_argument("--out_png", default="layer2_eq_curve.png")
    a = ap.parse_args(argv)
    freqs, delta0, delta_s, anchor, _, _, _ = analyze(
        a.base, a.target, sr=a.sr, max_minutes=a.max_minutes, n_fft=a.n_fft, hop=a.hop,
        music_dbfs=a.music_dbfs, anchor_lo=a.anchor_lo, anchor_hi=a.anchor_hi,
        clamp_db=a.clamp_db, smooth_bins=a.smooth_bins)
    out = np.stack([freqs, delta0, delta_s], axis=1)
    np.savetxt(a.out_csv, out, delimiter=",", header="freq_hz,delta_db_raw,delta_db_smooth",
               comments="")
    print(f"[SAVED] {a.out_csv}")
    print(f"[INFO] anchor(median {a.anchor_lo}-{a.anchor_hi}Hz) = {anchor:+.2f} dB (removed)")
    _plot(a.out_png, freqs, delta0, delta_s, a.sr, float(a.clamp_db))
    print(f"[SAVED] {a.out_png}")


if __name__ == "__main__":
    main()


__all__ = ["power_mono", "rms_dbfs", "find_delay_by_corr", "stft_logpower_median", "eq_tail",
           "analyze", "main"]
