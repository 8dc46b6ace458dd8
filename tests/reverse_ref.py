"""numpy statement of the parameter-recovery tools (reverse_engineer_params,
verify_tilt_amplitude): the per-frame arithmetic with a
``dtype`` argument (float32: as the reference computes it with numpy >= 2, where
the rfft of a float32 frame is complex64; float64: the yardstick), and the two
scripts' host logic as text.  Independent of the package under test."""
from __future__ import annotations

import io

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

EPS = 1e-12
SR, N_FFT, HOP = 48000, 4096, 2048
LEVEL_BINS = [(-70, -60), (-60, -55), (-55, -50), (-50, -45), (-45, -40), (-40, -35),
              (-35, -30), (-30, -25), (-25, -20), (-20, -15), (-15, -10)]
HIST_BINS = [(-40, -30), (-30, -20), (-20, -10), (-10, 0), (0, 10), (10, 20), (20, 30), (30, 40)]
TEST_FREQS = [250, 500, 1000, 2000, 4000, 8000]
SLAB = 16   # tm_analysis.hip kSlabFrames


def power_mono(x_lr, dtype=np.float32):
    x = np.asarray(x_lr, np.float32).astype(dtype)
    p = dtype(0.5) * (x[:, 0] ** 2 + x[:, 1] ** 2)
    return np.sqrt(p + dtype(EPS))


def n_frames(n, n_fft, hop):
    return 1 + (n - n_fft) // hop


def find_delay(x, y, sr=SR, ds_sr=2000):
    """find_delay_xcorr of both scripts (scipy, on the host)."""
    from scipy.signal import fftconvolve, resample_poly
    bm, cm = power_mono(x), power_mono(y)
    b = resample_poly(bm - bm.mean(), ds_sr, sr).astype(np.float32)
    c = resample_poly(cm - cm.mean(), ds_sr, sr).astype(np.float32)
    k = int(np.argmax(fftconvolve(c, b[::-1], mode="full")))
    return int(round((k - (len(b) - 1)) * (sr / ds_sr)))


def align_audio(x, y, delay):
    if delay > 0:
        y = y[delay:]
    elif delay < 0:
        x = x[-delay:]
    n = min(len(x), len(y))
    return x[:n], y[:n]


def frame_levels(x, n_fft=N_FFT, hop=HOP):
    """float32 20 log10(sqrt(mean(m m) + EPS) + EPS) per frame, numpy's own sums."""
    m = power_mono(x)
    F = max(0, n_frames(len(m), n_fft, hop))
    out = np.zeros(F, np.float32)
    for i in range(F):
        fr = m[i * hop:i * hop + n_fft]
        out[i] = 20 * np.log10(np.sqrt(np.mean(fr * fr) + EPS) + EPS)
    return out


def diff_rows(x, y, n_fft, hop, dtype=np.float32, idx=None):
    """-> (d [F, n_fft/2+1], |A|, |B|) in ``dtype``: d = 20 log10(|B| + EPS) -
    20 log10(|A| + EPS), A / B the spectra of win * power_mono(x / y)."""
    win = np.hanning(n_fft).astype(np.float32).astype(dtype)
    F = max(0, n_frames(len(x), n_fft, hop))
    idx = np.arange(F) if idx is None else np.asarray(idx)
    out = []
    for s in (x, y):
        m = power_mono(s, dtype)
        fr = sliding_window_view(m, n_fft)[::hop][:F][idx]
        mag = np.abs(np.fft.rfft(fr * win, axis=1))
        assert mag.dtype == dtype
        out.append(mag)
    A, B = out
    d = dtype(20) * np.log10(B + dtype(EPS)) - dtype(20) * np.log10(A + dtype(EPS))
    assert d.dtype == dtype
    return d, A, B


def band_range(freqs, f1, f2):
    i = np.nonzero((freqs >= f1) & (freqs < f2))[0]
    return (int(i[0]), int(i[-1]) + 1) if len(i) else (0, 0)


def tilts(d, lo, hi):
    """compute_tilt_index per row, in d's dtype (np.mean of a 1-D slice)."""
    out = np.zeros(len(d), d.dtype)
    for i, row in enumerate(d):
        out[i] = np.mean(row[hi[0]:hi[1]]) - np.mean(row[lo[0]:lo[1]])
    return out


def slab_mean(rows, frames=None):
    """The device's documented order over float32 rows: float64 sums in list
    order inside slabs of SLAB list entries, the slabs in ascending order, one
    division by the list's length."""
    rows = np.asarray(rows)
    frames = np.arange(len(rows)) if frames is None else np.asarray(frames, np.int64)
    nb = rows.shape[1]
    if len(frames) == 0:
        return np.full(nb, np.nan)
    total = np.zeros(nb)
    for s0 in range(0, len(frames), SLAB):
        part = np.zeros(nb)
        for f in frames[s0:s0 + SLAB]:
            part = part + rows[f].astype(np.float64)
        total = total + part
    return total / len(frames)


# ---------------------------------------------------------------------------
# reverse_engineer_params: the text after the file header
# ---------------------------------------------------------------------------

def reverse_table(x, y, delay, sr=SR, n_fft=N_FFT, hop=HOP, dtype=np.float32):
    xa, ya = align_audio(x, y, delay)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    d, _, _ = diff_rows(xa, ya, n_fft, hop, dtype)
    t = tilts(d, band_range(freqs, 200, 500), band_range(freqs, 2000, 6000))
    return dict(n=len(xa), levels=frame_levels(xa, n_fft, hop), tilts=t)


def reverse_counts(levels, tilt):
    return dict(level_bins=[int(np.count_nonzero((lo <= levels) & (levels < hi)))
                            for lo, hi in LEVEL_BINS],
                c1=int(np.count_nonzero(tilt < -5)), c2=int(np.count_nonzero(tilt > 5)),
                hist=[int(np.count_nonzero((lo <= tilt) & (tilt < hi))) for lo, hi in HIST_BINS])


def reverse_text(delay, n, levels, tilt, sr=SR, n_fft=N_FFT, hop=HOP):
    """stdout of analyze_device_params from the delay estimate on."""
    o = io.StringIO()

    def p(s=""):
        o.write(s + "\n")
    F = len(levels)
    p("\n正在计算对齐延迟...")
    p(f"延迟: {delay} samples ({delay/sr*1000:.2f} ms)")
    p(f"对齐后长度: {n} samples ({n/sr:.2f} sec)")
    p(f"\n分析帧数: {F}")
    p("\n正在逐帧分析...")
    for i in range(F):
        if (i + 1) % 5000 == 0:
            p(f"  已处理 {i+1}/{F} 帧...")
    p("\n分析完成!")
    p("\n" + "=" * 70)
    p("统计分析结果")
    p("=" * 70)
    p("\n按输入电平分组的倾斜指数统计:")
    p("-" * 60)
    p(f"{'电平范围':<15} {'平均倾斜':<12} {'标准差':<10} {'帧数':<8} {'状态'}")
    p("-" * 60)
    for lo, hi in LEVEL_BINS:
        t = [tilt[i] for i in range(F) if lo <= levels[i] < hi]
        if len(t) > 0:
            avg, std = np.mean(t), np.std(t)
            p(f"{lo:>3}~{hi:<3} dBFS   {avg:>+8.1f} dB   {std:>6.1f}    {len(t):<6}   "
              f"{'C1' if avg < 0 else 'C2'}")
    p("\n" + "-" * 60)
    p("Gate 阈值估计:")
    c1 = [levels[i] for i in range(F) if tilt[i] < -5]
    c2 = [levels[i] for i in range(F) if tilt[i] > 5]
    if len(c1) > 0 and len(c2) > 0:
        c1_max, c2_min = max(c1), min(c2)
        p(f"  C1 帧数: {len(c1)} (倾斜 < -5dB)")
        p(f"  C2 帧数: {len(c2)} (倾斜 > +5dB)")
        p(f"  C1 最大电平: {c1_max:.1f} dBFS")
        p(f"  C2 最小电平: {c2_min:.1f} dBFS")
        p(f"  估计 Gate 阈值: {(c1_max + c2_min)/2:.1f} dBFS")
    else:
        p("  无法估计Gate阈值 - 未检测到明显的C1/C2分离")
        p(f"  C1 帧数 (倾斜<-5dB): {len(c1)}")
        p(f"  C2 帧数 (倾斜>+5dB): {len(c2)}")
    p("\n倾斜指数分布:")
    for lo, hi in HIST_BINS:
        count = sum(1 for t in tilt if lo <= t < hi)
        pct = count / F * 100
        p(f"  {lo:>+3}~{hi:>+3} dB: {count:>5} ({pct:>5.1f}%) {'#' * int(pct / 2)}")
    return o.getvalue()


def reverse_csv(levels, tilt, sr=SR, hop=HOP):
    """The CSV's text (csv.writer's line ends)."""
    lines = ["frame,time_sec,inp_level_dbfs,tilt_db"]
    for i in range(len(levels)):
        lines.append(f"{i},{i * hop / sr:.3f},{levels[i]:.2f},{tilt[i]:.2f}")
    return "\r\n".join(lines) + "\r\n"


# ---------------------------------------------------------------------------
# verify_tilt_amplitude: the text after the banner
# ---------------------------------------------------------------------------

def amplitude(x, y, delay, sr=SR, n_fft=N_FFT, hop=HOP, dtype=np.float32):
    """-> dict(n_c1, n_c2, c1, c2 (frame lists)[, c1_avg, c2_avg, c1_tilt,
    c2_tilt]); float32: np.mean of the list of float32 rows, as the reference;
    float64: the float64 mean of float64 rows."""
    xa, ya = align_audio(x, y, delay)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    levels = frame_levels(xa, n_fft, hop)
    c1 = np.nonzero(levels < -45)[0]
    c2 = np.nonzero(levels > -30)[0]
    R = dict(delay=delay, n_c1=len(c1), n_c2=len(c2), c1=c1, c2=c2)
    if len(c1) > 10 and len(c2) > 10:
        for k, idx in (("c1", c1), ("c2", c2)):
            d, _, _ = diff_rows(xa, ya, n_fft, hop, dtype, idx)
            avg = np.mean(list(d), axis=0)
            R[k + "_avg"] = avg
            b = [band_range(freqs, 200, 300), band_range(freqs, 3500, 4500)]
            R[k + "_tilt"] = np.mean(avg[b[1][0]:b[1][1]]) - np.mean(avg[b[0][0]:b[0][1]])
    return R


def amplitude_text(R, sr=SR, n_fft=N_FFT):
    o = io.StringIO()

    def p(s=""):
        o.write(s + "\n")
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    p(f"Delay: {R['delay']} samples")
    p(f"\nC1 frames (level < -45 dBFS): {R['n_c1']}")
    p(f"C2 frames (level > -30 dBFS): {R['n_c2']}")
    if "c1_avg" in R:
        for k, title, th in (("c1", "C1 状态 (安静段落) 频谱增益:", "-30"),
                             ("c2", "C2 状态 (响亮段落) 频谱增益:", "+30")):
            p("\n" + "=" * 70)
            p(title)
            p("-" * 50)
            for f in TEST_FREQS:
                p(f"  {f:5d} Hz: {R[k + '_avg'][np.argmin(np.abs(freqs - f))]:+.1f} dB")
            p(f"\n  倾斜 (4kHz - 250Hz): {R[k + '_tilt']:+.1f} dB")
            p(f"  理论值: {th} dB")
        p("\n" + "=" * 70)
        p("总结:")
        p("-" * 50)
        p(f"  C1 实测倾斜: {R['c1_tilt']:+.1f} dB (理论 -30 dB)")
        p(f"  C2 实测倾斜: {R['c2_tilt']:+.1f} dB (理论 +30 dB)")
        p(f"  C1-C2 差异: {R['c1_tilt'] - R['c2_tilt']:.1f} dB (理论 -60 dB)")
    return o.getvalue()


def rule_bound_db(e32):
    """The project's rule in dB: 8 * max(the float32 statement's own error, the
    floor 20 / ln 10 * 2^-23)."""
    return 8 * max(float(e32), 20 / np.log(10) * 2.0 ** -23)
