"""Recover the device's processing parameters from an input file and the
device's recording of it — MI355X drop-in for src/reverse_engineer_params.py
(the calibration family).

Same function names, flags, defaults, prints and CSV as the reference; the
per-sample and per-frame work runs in ``libtomatis_hip.so``:

  reference (file:line)             here
  --------------------------------- ---------------------------------------------
  find_delay_xcorr :35-45           align.find_delay_full (tm_align.hip envelope,
                                    tm_fftcorr.hip FFT correlation, arg-max)
  align_audio :47-54                two row slices of the resident tensors
  power_mono + rms_dbfs of a frame  tomatis_an_frame_r (POWER_MONO, bit-exact r);
  :122-123                          the float32 20*log10(r + EPS) on the host
  compute_frame_spectrum twice,     tomatis_an_pair_tilt (tm_analysis.hip
  diff_spec, compute_tilt_index     k_an_pair_tilt): one transform per frame, the
  :126-136                          two band means leave the workgroup
  level-bin table, gate estimate,   host: the reference's numpy and formats over
  histogram, CSV :150-219           the F levels and tilts

The reference hard-codes SR, N_FFT and HOP and ignores the files' rates; they
are keyword defaults of ``analyze`` here, and the files' rates are ignored too.

Precision: the reference's spectra are float32 (with numpy >= 2 the rfft of a
float32 frame is complex64) and so are its two band means; here the bins are
float32 and each band mean is a float64 sum, the tilt is rounded to float32
once.  The levels are the reference's bits.

``analyze()`` is ``analyze_device_params()`` minus the files and the CSV.
"""
from __future__ import annotations

import csv

import numpy as np

from . import align, analysis, audio_io
from .calibrate_to_baseline_v2 import frame_levels

EPS = 1e-12
SR = 48000
N_FFT = 4096
HOP = 2048
LOW_BAND, HIGH_BAND = (200, 500), (2000, 6000)
LEVEL_BINS = [(-70, -60), (-60, -55), (-55, -50), (-50, -45),
              (-45, -40), (-40, -35), (-35, -30), (-30, -25),
              (-25, -20), (-20, -15), (-15, -10)]
HIST_BINS = [(-40, -30), (-30, -20), (-20, -10), (-10, 0),
             (0, 10), (10, 20), (20, 30), (30, 40)]


def power_mono(x_lr):
    """reverse_engineer_params.py:26-29 (host, elementwise)."""
    p = 0.5 * (x_lr[:, 0]**2 + x_lr[:, 1]**2)
    return np.sqrt(p + EPS)


def rms_dbfs(x):
    """reverse_engineer_params.py:31-33 (host)."""
    return 20 * np.log10(np.sqrt(np.mean(x*x) + EPS) + EPS)


def find_delay_xcorr(base, cand, sr=SR, ds_sr=2000):
    """reverse_engineer_params.py:35-45: compare_audio's full-mode correlation.
    ``base`` / ``cand`` are the stereo ``[n, 2]`` signals (arrays, cuda tensors
    or paths), or the reference's own 1-D power-mono vectors."""
    if not isinstance(base, str) and getattr(base, "ndim", 0) == 1:
        return align.delay_full_mono(base, cand, sr, ds_sr)
    return align.find_delay_full(base, cand, sr=sr, ds_sr=ds_sr)


def align_audio(base_lr, cand_lr, delay):
    """reverse_engineer_params.py:47-54; arrays or resident tensors (row slices)."""
    if delay > 0:
        cand_lr = cand_lr[delay:]
    elif delay < 0:
        base_lr = base_lr[-delay:]
    n = min(len(base_lr), len(cand_lr))
    return base_lr[:n], cand_lr[:n]


def compute_tilt_index(spec_db, freqs, fc=1000):
    """reverse_engineer_params.py:62-76 (host, one row)."""
    low_mask = (freqs >= LOW_BAND[0]) & (freqs < LOW_BAND[1])
    high_mask = (freqs >= HIGH_BAND[0]) & (freqs < HIGH_BAND[1])
    low_avg = np.mean(spec_db[low_mask])
    high_avg = np.mean(spec_db[high_mask])
    return high_avg - low_avg


def band_range(freqs, f1, f2):
    """[b0, b1): the bins of the mask (freqs >= f1) & (freqs < f2); (0, 0) when
    there is none (its mean is NaN, as the reference's)."""
    idx = np.nonzero((freqs >= f1) & (freqs < f2))[0]
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def frame_tilts(xd, yd, sr, n_fft, hop):
    """np.float32 tilt of every frame of an aligned resident pair (:126-136)."""
    freqs = np.fft.rfftfreq(n_fft, 1/sr)
    means, _ = analysis.pair_tilt(xd, yd, n_fft, hop, band_range(freqs, *LOW_BAND),
                                  band_range(freqs, *HIGH_BAND))
    m = means.cpu().numpy()
    return (m[:, 1] - m[:, 0]).astype(np.float32)


def report(levels, tilts, log=print):
    """The statistics of :150-209 over the float32 levels and tilts."""
    log("\n" + "=" * 70)
    log("统计分析结果")
    log("=" * 70)

    log("\n按输入电平分组的倾斜指数统计:")
    log("-" * 60)
    log(f"{'电平范围':<15} {'平均倾斜':<12} {'标准差':<10} {'帧数':<8} {'状态'}")
    log("-" * 60)

    for lo, hi in LEVEL_BINS:
        in_bin = (lo <= levels) & (levels < hi)
        n_in = int(np.count_nonzero(in_bin))
        if n_in > 0:
            avg_tilt = np.mean(tilts[in_bin])
            std_tilt = np.std(tilts[in_bin])
            state = "C1" if avg_tilt < 0 else "C2"
            log(f"{lo:>3}~{hi:<3} dBFS   {avg_tilt:>+8.1f} dB   {std_tilt:>6.1f}    {n_in:<6}   {state}")

    log("\n" + "-" * 60)
    log("Gate 阈值估计:")

    c1 = tilts < -5
    c2 = tilts > 5
    n1, n2 = int(np.count_nonzero(c1)), int(np.count_nonzero(c2))

    if n1 > 0 and n2 > 0:
        c1_max = max(levels[c1])
        c2_min = min(levels[c2])

        log(f"  C1 帧数: {n1} (倾斜 < -5dB)")
        log(f"  C2 帧数: {n2} (倾斜 > +5dB)")
        log(f"  C1 最大电平: {c1_max:.1f} dBFS")
        log(f"  C2 最小电平: {c2_min:.1f} dBFS")
        log(f"  估计 Gate 阈值: {(c1_max + c2_min)/2:.1f} dBFS")
    else:
        log("  无法估计Gate阈值 - 未检测到明显的C1/C2分离")
        log(f"  C1 帧数 (倾斜<-5dB): {n1}")
        log(f"  C2 帧数 (倾斜>+5dB): {n2}")

    log("\n倾斜指数分布:")
    for lo, hi in HIST_BINS:
        count = int(np.count_nonzero((lo <= tilts) & (tilts < hi)))
        pct = count / len(tilts) * 100
        bar = "#" * int(pct / 2)
        log(f"  {lo:>+3}~{hi:>+3} dB: {count:>5} ({pct:>5.1f}%) {bar}")


def analyze(x, y, *, sr=SR, n_fft=N_FFT, hop=HOP, log=print):
    """analyze_device_params (:94-209) on two stereo signals (arrays or resident
    cuda tensors): returns the frame table as arrays, dict(delay, frame, time,
    inp_level, tilt)."""
    xd, yd = align._stereo_dev(x), align._stereo_dev(y)
    assert xd.dim() == 2 and xd.shape[1] == 2 and yd.dim() == 2 and yd.shape[1] == 2

    log("\n正在计算对齐延迟...")
    delay = find_delay_xcorr(xd, yd, sr=sr)
    log(f"延迟: {delay} samples ({delay/sr*1000:.2f} ms)")

    xa, ya = align_audio(xd, yd, delay)
    log(f"对齐后长度: {len(xa)} samples ({len(xa)/sr:.2f} sec)")

    n_frames = 1 + (len(xa) - n_fft) // hop

    log(f"\n分析帧数: {n_frames}")
    log("\n正在逐帧分析...")

    levels = frame_levels(xa, n_fft, hop)
    tilts = frame_tilts(xa, ya, sr, n_fft, hop) if n_frames > 0 else np.zeros(0, np.float32)
    for done in range(5000, n_frames + 1, 5000):
        log(f"  已处理 {done}/{n_frames} 帧...")

    log("\n分析完成!")
    report(levels, tilts, log)

    frame = np.arange(max(0, n_frames), dtype=np.int64)
    return dict(delay=delay, frame=frame, time=frame * hop / sr, inp_level=levels, tilt=tilts)


def write_csv(out_csv, table):
    """:212-218."""
    with open(out_csv, 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['frame', 'time_sec', 'inp_level_dbfs', 'tilt_db'])
        for i, t, lv, ti in zip(table["frame"].tolist(), table["time"].tolist(),
                                table["inp_level"], table["tilt"]):
            writer.writerow([i, f"{t:.3f}", f"{lv:.2f}", f"{ti:.2f}"])


def analyze_device_params(input_path, output_path, out_csv=None, *, sr=SR, n_fft=N_FFT, hop=HOP):
    """reverse_engineer_params.py:78-221."""
    print("=" * 70)
    print("Tomatis 设备参数反推分析")
    print("=" * 70)

    print(f"\n输入文件: {input_path}")
    print(f"输出文件: {output_path}")

    inp_lr, _ = audio_io.read(input_path)
    out_lr, _ = audio_io.read(output_path)

    print(f"\n输入长度: {len(inp_lr)} samples ({len(inp_lr)/sr:.2f} sec)")
    print(f"输出长度: {len(out_lr)} samples ({len(out_lr)/sr:.2f} sec)")

    table = analyze(inp_lr, out_lr, sr=sr, n_fft=n_fft, hop=hop)

    if out_csv:
        write_csv(out_csv, table)
        print(f"\n详细数据已保存: {out_csv}")

    return [{'frame': i, 'time': t, 'inp_level': lv, 'tilt': ti}
            for i, t, lv, ti in zip(table["frame"].tolist(), table["time"].tolist(),
                                    table["inp_level"], table["tilt"])]


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="反推Tomatis设备参数")
    ap.add_argument("-i", "--input", required=True, help="原始输入文件")
    ap.add_argument("-o", "--output", required=True, help="设备输出文件")
    ap.add_argument("--csv", default=None, help="输出CSV文件路径")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    analyze_device_params(args.input, args.output, args.csv)


if __name__ == "__main__":
    main()


__all__ = ["power_mono", "rms_dbfs", "find_delay_xcorr", "align_audio", "compute_tilt_index",
           "band_range", "frame_tilts", "report", "analyze", "write_csv",
           "analyze_device_params", "main"]
