"""Measure the tilt filter's actual gain curves in the two gate states from an
input file and the device's recording of it — MI355X drop-in for
src/verify_tilt_amplitude.py (the calibration family).

Same function names, defaults and prints as the reference; the per-sample and
per-frame work runs in ``libtomatis_hip.so``:

  reference (file:line)             here
  --------------------------------- ---------------------------------------------
  find_delay_xcorr :26-33           align.find_delay_full (tm_align.hip envelope,
                                    tm_fftcorr.hip FFT correlation, arg-max)
  align_audio :35-41                two row slices of the resident tensors
  inp_level of a frame :76-79       tomatis_an_frame_r (POWER_MONO, bit-exact r);
                                    the float32 20*log10(r + EPS) on the host
  level classes :89-92              host: float32 comparisons over the F levels
  diff_db of a frame, and           tomatis_an_pair_diff_mean (tm_analysis.hip
  np.mean(diffs, axis=0) :82-87,    k_an_pair_diff_mean), one call per class with
  :98-99                            that class's frame list
  key-frequency gains,              host: the reference's numpy on n_fft / 2 + 1
  band_power_db :101-136            bins

Precision: the reference's rows are float32 and numpy adds them in float32 in
frame order; here the bins are float32 and the mean over frames is a float64
sum in slabs of 16 list entries.  The levels, and so the classes
and their counts, are the reference's bits.

``analyze()`` is ``analyze_tilt_detail()`` minus the files; ``main()`` takes the
two paths as optional arguments (the reference's are fixed names).
"""
from __future__ import annotations

import numpy as np

from . import align, analysis, audio_io
from .calibrate_to_baseline_v2 import frame_levels

EPS = 1e-12
SR = 48000
N_FFT = 4096
HOP = 2048
TEST_FREQS = [250, 500, 1000, 2000, 4000, 8000]
DEFAULT_INPUT, DEFAULT_OUTPUT = "D MNF.flac", "Tomatis_D_30m_declick.flac"


def power_mono(x_lr):
    """verify_tilt_amplitude.py:22-24 (host, elementwise)."""
    p = 0.5 * (x_lr[:, 0]**2 + x_lr[:, 1]**2)
    return np.sqrt(p + EPS)


def find_delay_xcorr(base, cand, sr=SR, ds_sr=2000):
    """verify_tilt_amplitude.py:26-33: compare_audio's full-mode correlation.
    ``base`` / ``cand`` are the stereo ``[n, 2]`` signals (arrays, cuda tensors
    or paths), or the reference's own 1-D power-mono vectors."""
    if not isinstance(base, str) and getattr(base, "ndim", 0) == 1:
        return align.delay_full_mono(base, cand, sr, ds_sr)
    return align.find_delay_full(base, cand, sr=sr, ds_sr=ds_sr)


def align_audio(base_lr, cand_lr, delay):
    """verify_tilt_amplitude.py:35-41; arrays or resident tensors (row slices)."""
    if delay > 0:
        cand_lr = cand_lr[delay:]
    elif delay < 0:
        base_lr = base_lr[-delay:]
    n = min(len(base_lr), len(cand_lr))
    return base_lr[:n], cand_lr[:n]


def band_power_db(spec_db, freqs, f1, f2):
    """verify_tilt_amplitude.py:43-46 (host)."""
    mask = (freqs >= f1) & (freqs < f2)
    return np.mean(spec_db[mask])


def _state(title, avg, freqs, theory, log):
    log("\n" + "=" * 70)
    log(title)
    log("-" * 50)
    for f in TEST_FREQS:
        idx = np.argmin(np.abs(freqs - f))
        gain = avg[idx]
        log(f"  {f:5d} Hz: {gain:+.1f} dB")
    tilt = band_power_db(avg, freqs, 3500, 4500) - band_power_db(avg, freqs, 200, 300)
    log(f"\n  倾斜 (4kHz - 250Hz): {tilt:+.1f} dB")
    log(f"  理论值: {theory} dB")
    return tilt


def analyze(x, y, *, sr=SR, n_fft=N_FFT, hop=HOP, log=print):
    """analyze_tilt_detail (:57-136) on two stereo signals (arrays or resident
    cuda tensors): returns dict(delay, n_c1, n_c2), and where both classes hold
    more than 10 frames (the reference's ``if``) also c1_avg, c2_avg (float64
    [n_fft/2+1]), c1_tilt and c2_tilt."""
    xd, yd = align._stereo_dev(x), align._stereo_dev(y)
    assert xd.dim() == 2 and xd.shape[1] == 2 and yd.dim() == 2 and yd.shape[1] == 2

    delay = find_delay_xcorr(xd, yd, sr=sr)
    log(f"Delay: {delay} samples")

    xa, ya = align_audio(xd, yd, delay)
    freqs = np.fft.rfftfreq(n_fft, 1/sr)

    levels = frame_levels(xa, n_fft, hop)
    c1 = np.nonzero(levels < -45)[0]   # 低电平帧 (< -45 dBFS)
    c2 = np.nonzero(levels > -30)[0]   # 高电平帧 (> -30 dBFS)

    log(f"\nC1 frames (level < -45 dBFS): {len(c1)}")
    log(f"C2 frames (level > -30 dBFS): {len(c2)}")
    res = dict(delay=delay, n_c1=len(c1), n_c2=len(c2))

    if len(c1) > 10 and len(c2) > 10:
        c1_avg = analysis.pair_diff_mean(xa, ya, n_fft, hop, c1).cpu().numpy()
        c2_avg = analysis.pair_diff_mean(xa, ya, n_fft, hop, c2).cpu().numpy()

        t1 = _state("C1 状态 (安静段落) 频谱增益:", c1_avg, freqs, "-30", log)
        t2 = _state("C2 状态 (响亮段落) 频谱增益:", c2_avg, freqs, "+30", log)

        log("\n" + "=" * 70)
        log("总结:")
        log("-" * 50)
        log(f"  C1 实测倾斜: {t1:+.1f} dB (理论 -30 dB)")
        log(f"  C2 实测倾斜: {t2:+.1f} dB (理论 +30 dB)")
        log(f"  C1-C2 差异: {t1 - t2:.1f} dB (理论 -60 dB)")
        res.update(c1_avg=c1_avg, c2_avg=c2_avg, c1_tilt=float(t1), c2_tilt=float(t2))
    return res


def analyze_tilt_detail(input_path, output_path, *, sr=SR, n_fft=N_FFT, hop=HOP):
    """verify_tilt_amplitude.py:48-136."""
    print("=" * 70)
    print("倾斜滤波器增益幅度验证")
    print("=" * 70)

    inp_lr, _ = audio_io.read(input_path)
    out_lr, _ = audio_io.read(output_path)
    return analyze(inp_lr, out_lr, sr=sr, n_fft=n_fft, hop=hop)


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="验证倾斜滤波器的实际增益幅度")
    ap.add_argument("input", nargs="?", default=DEFAULT_INPUT, help="原始输入文件")
    ap.add_argument("output", nargs="?", default=DEFAULT_OUTPUT, help="设备输出文件")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    analyze_tilt_detail(args.input, args.output)


if __name__ == "__main__":
    main()


__all__ = ["power_mono", "find_delay_xcorr", "align_audio", "band_power_db", "analyze",
           "analyze_tilt_detail", "main"]
