"""Self-contained acceptance validator for a +-15 dB output — MI355X drop-in for
src/verify_tomatis_15db_v2.py (workflow: "is this processed file acceptable";
SURVEY.md §8 row f9).  It re-solves the gate threshold from the input (target
C2 share 50 %), then judges the output: engineering checks, conditional spectra
anchored to 900-1100 Hz against the theoretical tilt curves, and the tilt index.

Same function names, flags, defaults, printed lines, CSV header and number
formats, report text (``<prefix>_report.txt``) and PNGs as the reference; the
PCM is uploaded once and everything per sample or per bin runs in
``libtomatis_hip.so``:

  reference (file:line)                 here
  ------------------------------------- -----------------------------------------
  check_engineering :63-94              audio_io.info; tomatis_absmax (peak);
                                        tomatis_sum_f64 (DC mean, float64 sum)
  compute_frame_levels :101-123         zero padding on the device,
                                        tomatis_an_frame_r (bit-exact r), the
                                        reference's ``20 log10(r + EPS)`` on the host
  simulate_gate_with_threshold          tomatis_cal_gate_grid, one candidate, frame
  :126-152                              indices as starts (up-delay in frames)
  find_optimal_threshold :155-199       at most 30 dependent launches of that scan;
                                        the host keeps T_low / T_high and the counts
  compute_conditional_spectrum_v2       tomatis_an_anchored_ratio (rows anchored in
  :270-369                              the workgroup), tomatis_an_frame_median per
                                        class; percentile, stable classes and the
                                        final ``20 log10`` over bins on the host
  compute_tilt_index :421-485           tomatis_an_pair_band_energy; the host keeps
                                        the per-frame ``10 log10(E_hi / E_lo + EPS)``
  sections C + D in ``verify``          tomatis_an_verify_pair: both from one
                                        transform per (frame, channel)
  analyze_gate_stats, metrics, report   host: numpy on per-frame lists and bins

``verify(x, y, sr, ...)`` is ``main()`` minus argparse and the file reads; it
takes numpy arrays or resident cuda tensors.  There is no CPU fallback: without
a device every spectrum, level or scan raises.

Two places where the reference would raise and this module goes on: a ``y``
shorter than ``x`` (by at most ``n_fft // 2``) is zero-extended in the tilt index
as the reference's padding does in the conditional spectrum, and ``states`` may
be an integer array (1 / 2) as well as a list of ``'C1'`` / ``'C2'``.

One place where the reference goes on and this module raises: the gate scan
(``simulate_gate_with_threshold``, ``find_optimal_threshold``) takes levels that
are float32 values, which is what ``compute_frame_levels`` returns here and in
the reference (``20 log10(r + EPS)`` of a float32 ``r``); the kernel compares in
float32 with thresholds rounded towards the level side, which reproduces the
float64 comparison for such levels only.  Other float64 levels raise a
``ValueError`` instead of being rounded silently.
"""
from __future__ import annotations

import argparse
import csv
import sys

import numpy as np

from . import analysis, audio_io
from .analysis import find_stable_frames  # noqa: F401  (reference name, :254-267)
from .dsp import build_tilt_gain_db  # noqa: F401  (reference name, :42-56)

EPS = 1e-12
# fuse sections C and D into one launch (measured faster than two)
FUSED = True


def rms_dbfs(x_mono: np.ndarray) -> float:
    """verify_tomatis_15db_v2.py:36-39 (host, one frame)."""
    r = np.sqrt(np.mean(x_mono * x_mono) + EPS)
    return float(20.0 * np.log10(r + EPS))


# ---------------------------------------------------------------------------
# A. engineering checks
# ---------------------------------------------------------------------------

def _engineering(sr_in, ch_in, frames_in, sr_out, ch_out, frames_out, yd):
    """:63-94 on the file facts and the resident output."""
    results = {}
    results['sr_in'] = sr_in
    results['sr_out'] = sr_out
    results['sr_match'] = sr_in == sr_out
    results['ch_in'] = ch_in
    results['ch_out'] = ch_out
    results['ch_match'] = ch_in == ch_out
    results['frames_in'] = frames_in
    results['frames_out'] = frames_out
    results['frames_match'] = frames_in == frames_out
    results['frames_diff'] = frames_out - frames_in
    peak = analysis.absmax(yd)
    results['peak'] = peak
    results['peak_safe'] = bool(peak < 0.98)
    results['peak_dbfs'] = 20 * np.log10(peak + EPS)
    dc_mean = analysis.sum_f64(yd) / max(1, yd.numel())  # float64 sum of the float32 samples
    results['dc_mean'] = dc_mean
    results['dc_safe'] = abs(dc_mean) < 0.001
    return results


def check_engineering(in_path, out_path):
    """:63-94: sample rate / channels / length / peak / DC offset of two files."""
    sr_in, ch_in, n_in = audio_io.info(in_path)
    sr_out, ch_out, n_out = audio_io.info(out_path)
    y, _ = audio_io.read(out_path)
    return _engineering(sr_in, ch_in, n_in, sr_out, ch_out, n_out, analysis._dev(y, ch=True))


# ---------------------------------------------------------------------------
# B. adaptive gate threshold
# ---------------------------------------------------------------------------

def compute_frame_levels(x, sr, n_fft, hop):
    """:101-123: RMS dBFS of every frame of the n_fft // 2-padded grid (device r)."""
    return analysis.padded_frame_levels(analysis._dev(x, ch=True), n_fft, hop)[0]


def _scan_of(levels):
    return analysis.GateScan(levels, np.arange(len(levels), dtype=np.int64))


def simulate_gate_with_threshold(levels, threshold_dbfs, hyst_db, up_delay_frames=0):
    """:126-152: the states ('C1' / 'C2') for one threshold (device scan)."""
    Ton = threshold_dbfs + hyst_db / 2
    Toff = threshold_dbfs - hyst_db / 2
    _, _, codes = _scan_of(levels).run(Ton, Toff, up_delay_frames, want_states=True)
    return analysis.state_names(codes)


def _find_optimal_threshold(scan, levels, hyst_db, target_c2_ratio, up_delay_frames):
    level_median = np.median(levels)
    T_low = np.min(levels) - 10
    T_high = np.max(levels) + 10
    best_T, best_ratio, best_diff = level_median, 0.0, 1.0
    for _ in range(30):
        T_mid = (T_low + T_high) / 2
        c2, _ = scan.run(T_mid + hyst_db / 2, T_mid - hyst_db / 2, up_delay_frames)
        c2_ratio = c2 / len(levels)
        diff = abs(c2_ratio - target_c2_ratio)
        if diff < best_diff:
            best_diff, best_T, best_ratio = diff, T_mid, c2_ratio
        if diff < 0.01:
            break
        if c2_ratio < target_c2_ratio:
            T_high = T_mid  # too little C2: lower the threshold
        else:
            T_low = T_mid
    return best_T, best_ratio


def find_optimal_threshold(levels, hyst_db, target_c2_ratio=0.5, up_delay_frames=0):
    """:155-199: bisection on the threshold until the C2 share is within 1 % of the
    target, at most 30 steps -> (optimal_threshold, achieved_c2_ratio)."""
    levels = np.asarray(levels, np.float64)
    return _find_optimal_threshold(_scan_of(levels), levels, hyst_db, target_c2_ratio,
                                   up_delay_frames)


def _runs(codes):
    """Run lengths of a state sequence (n >= 1)."""
    cut = np.nonzero(codes[1:] != codes[:-1])[0] + 1
    return np.diff(np.concatenate([[0], cut, [len(codes)]]))


def analyze_gate_stats(states, levels, sr, hop):
    """:202-247."""
    codes = analysis.state_codes(states)
    n = len(codes)
    if n == 0:
        return {}
    levels = np.asarray(levels)
    c2_count = int(np.count_nonzero(codes == 2))
    run_lengths = _runs(codes)
    switch_count = len(run_lengths) - 1
    short_runs = int(np.count_nonzero(run_lengths <= 3))
    duration_min = n * hop / sr / 60
    c1_levels, c2_levels = levels[:n][codes == 1], levels[:n][codes == 2]
    return {
        'total_frames': n,
        'duration_min': duration_min,
        'c2_count': c2_count,
        'c2_ratio': c2_count / n,
        'switch_count': switch_count,
        'switches_per_min': switch_count / duration_min if duration_min > 0 else 0,
        'run_min': int(run_lengths.min()),
        'run_max': int(run_lengths.max()),
        'run_median': np.median(run_lengths),
        'short_runs': short_runs,
        'short_run_ratio': short_runs / len(run_lengths),
        'c1_level_mean': np.mean(c1_levels) if len(c1_levels) else 0,
        'c2_level_mean': np.mean(c2_levels) if len(c2_levels) else 0,
    }


# ---------------------------------------------------------------------------
# C. conditional spectra, anchored to a band
# ---------------------------------------------------------------------------

def _conditional(rows, F, sr, codes, levels, n_fft, level_percentile):
    """:290-369 from the anchored rows of the F frames fully inside x."""
    import torch
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    nb = len(freqs)
    level_threshold = np.percentile(levels, level_percentile)
    cls = np.zeros(F, np.int8)
    sc = analysis.stable_classes(codes, margin=2)[:F]
    cls[:len(sc)] = sc
    loud = np.zeros(F, bool)
    m = min(F, len(levels))
    loud[:m] = ~(np.asarray(levels)[:m] < level_threshold)
    out, used = [], []
    for v in (1, 2):
        mask = (cls == v) & loud
        cnt = int(np.count_nonzero(mask))
        used.append(cnt)
        if cnt:
            md = torch.from_numpy(mask.astype(np.uint8)).cuda()
            med = analysis.frame_median(rows, md, cnt).cpu().numpy()
            out.append(20 * np.log10(med + EPS))
        else:
            out.append(np.zeros(nb))
    return freqs, out[0], out[1], used[0], used[1]


def compute_conditional_spectrum_v2(x, y, sr, states, levels, n_fft, hop,
                                    level_percentile=10, anchor_band=(900, 1100)):
    """:270-369 -> (freqs, c1_db, c2_db, c1_used, c2_used): per stable frame at or
    above the level percentile the ratio mean_c|Y_c| / max(mean_c|X_c|, 1e-10)
    divided by its mean over the anchor band; the median over frames per class."""
    xd, yd = analysis.pair_on_device(x, y, n_fft // 2)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    anchor = analysis.band_bins(freqs, anchor_band[0], anchor_band[1])
    rows, _ = analysis.verify_spectra(xd, yd, n_fft, hop, anchor=anchor)
    return _conditional(rows, rows.shape[0], sr, analysis.state_codes(states), levels, n_fft,
                        level_percentile)


def compute_spectrum_metrics_v2(freqs, c1_db, c2_db, c1_theory, c2_theory, fc, gain_limit):
    """:372-414 (host: bins)."""
    metrics = {}
    f_lo_platform = fc * 2 ** (-gain_limit / 12)
    f_hi_platform = fc * 2 ** (gain_limit / 12)

    def rmse(meas, th, mask):
        return np.sqrt(np.mean((meas[mask] - th[mask]) ** 2))

    lo_mask = (freqs >= 100) & (freqs <= f_lo_platform * 0.8)
    if np.any(lo_mask):
        metrics['c1_lo_platform_rmse'] = rmse(c1_db, c1_theory, lo_mask)
        metrics['c2_lo_platform_rmse'] = rmse(c2_db, c2_theory, lo_mask)
        metrics['c1_lo_platform_mean'] = np.mean(c1_db[lo_mask])
        metrics['c2_lo_platform_mean'] = np.mean(c2_db[lo_mask])
    hi_mask = (freqs >= f_hi_platform * 1.2) & (freqs <= 10000)
    if np.any(hi_mask):
        metrics['c1_hi_platform_rmse'] = rmse(c1_db, c1_theory, hi_mask)
        metrics['c2_hi_platform_rmse'] = rmse(c2_db, c2_theory, hi_mask)
        metrics['c1_hi_platform_mean'] = np.mean(c1_db[hi_mask])
        metrics['c2_hi_platform_mean'] = np.mean(c2_db[hi_mask])
    slope_mask = (freqs >= f_lo_platform * 1.2) & (freqs <= f_hi_platform * 0.8)
    if np.any(slope_mask):
        metrics['c1_slope_rmse'] = rmse(c1_db, c1_theory, slope_mask)
        metrics['c2_slope_rmse'] = rmse(c2_db, c2_theory, slope_mask)
    fc_mask = (freqs >= 900) & (freqs <= 1100)
    if np.any(fc_mask):
        metrics['c1_fc_error'] = abs(np.mean(c1_db[fc_mask]))
        metrics['c2_fc_error'] = abs(np.mean(c2_db[fc_mask]))
    return metrics


# ---------------------------------------------------------------------------
# D. tilt index
# ---------------------------------------------------------------------------

def _tilt(be, F, codes, levels, level_percentile):
    """:435-485 from the band energies [F, 4] of the frames fully inside x."""
    level_threshold = np.percentile(levels, level_percentile)
    m = min(F, len(codes))
    e = be[:m]
    keep = ~(np.asarray(levels)[:m] < level_threshold)
    c = np.asarray(codes)[:m]

    def ti(lo, hi, ok):
        return 10 * np.log10(hi[ok] / lo[ok] + EPS)

    okx = keep & (e[:, 0] > EPS)
    oky = keep & (e[:, 2] > EPS)
    ti_y = np.full(m, np.nan, np.float32)
    ti_y[oky] = ti(e[:, 2], e[:, 3], oky)
    return {
        'input': ti(e[:, 0], e[:, 1], okx),
        'output': ti_y[oky],
        'c1': ti_y[oky & (c == 1)],
        'c2': ti_y[oky & (c != 1)],
    }


def _tilt_bands(sr, n_fft):
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    return (*analysis.band_bins(freqs, 200, 1000), *analysis.band_bins(freqs, 2000, 8000))


def compute_tilt_index(x, y, sr, states, levels, n_fft, hop, level_percentile=10):
    """:421-485: per frame at or above the level percentile
    10 log10(E(2-8 kHz) / E(200-1000 Hz) + EPS) of the input and of the output,
    the output's also per state."""
    xd, yd = analysis.pair_on_device(x, y, n_fft // 2)
    _, be = analysis.verify_spectra(xd, yd, n_fft, hop, bands=_tilt_bands(sr, n_fft))
    return _tilt(be.cpu().numpy(), be.shape[0], analysis.state_codes(states), levels,
                 level_percentile)


def analyze_tilt_index(ti_data):
    """:488-502."""
    results = {}
    for key in ['input', 'output', 'c1', 'c2']:
        arr = ti_data[key]
        if len(arr) > 0:
            results[f'{key}_mean'] = np.mean(arr)
            results[f'{key}_std'] = np.std(arr)
            results[f'{key}_n'] = len(arr)
    if 'c1_mean' in results and 'c2_mean' in results:
        results['ti_effect'] = results['c2_mean'] - results['c1_mean']
    return results


# ---------------------------------------------------------------------------
# the run
# ---------------------------------------------------------------------------

def _plots(a, R):
    """:739-814."""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        print('  matplotlib 未安装，跳过绘图')
        return
    import warnings
    with warnings.catch_warnings():
        # the titles are the reference's; a font without their glyphs draws boxes
        warnings.filterwarnings('ignore', message='Glyph .* missing from font')
        _draw(plt, a, R)


def _draw(plt, a, R):
    freqs, gain_limit, ti_data, ti_results = R['freqs'], R['gain_limit'], R['ti_data'], R['ti']
    fig, axes = plt.subplots(2, 1, figsize=(14, 10))
    for ax, name, col, meas, th, n_used in (
            (axes[0], 'C1', 'b', R['c1_db'], R['c1_theory'], R['c1_n']),
            (axes[1], 'C2', 'r', R['c2_db'], R['c2_theory'], R['c2_n'])):
        ax.semilogx(freqs, meas, col + '-', label=f'{name} measured', alpha=0.7, linewidth=1.5)
        ax.semilogx(freqs, th, col + '--', label=f'{name} theory', linewidth=2)
        ax.axhline(0, color='gray', linestyle=':', alpha=0.5)
        ax.axhline(gain_limit, color='green', linestyle=':', alpha=0.5)
        ax.axhline(-gain_limit, color='red', linestyle=':', alpha=0.5)
        ax.axvline(a.fc, color='orange', linestyle='--', alpha=0.7, label=f'fc={a.fc}Hz')
        ax.set_xlim(20, 20000)
        ax.set_ylim(-20, 20)
        ax.set_xlabel('Frequency (Hz)')
        ax.set_ylabel('Gain (dB)')
        ax.set_title(f'{name} 条件频谱 (n={n_used}, 剔除<p{a.level_percentile}能量帧)')
        ax.legend(loc='upper right')
        ax.grid(True, alpha=0.3)
    plt.tight_layout()
    spectrum_png = f'{a.out_prefix}_spectrum.png'
    plt.savefig(spectrum_png, dpi=150)
    print(f'  频谱图已保存: {spectrum_png}')
    plt.close()

    fig, axes = plt.subplots(1, 2, figsize=(14, 5))
    ax = axes[0]
    ax.hist(ti_data['input'], bins=50, alpha=0.5, label='Input', color='gray')
    ax.hist(ti_data['output'], bins=50, alpha=0.5, label='Output', color='blue')
    ax.set_xlabel('Tilt Index (dB)')
    ax.set_ylabel('Count')
    ax.set_title('Tilt Index: Input vs Output')
    ax.legend()
    ax.grid(True, alpha=0.3)
    ax = axes[1]
    if len(ti_data['c1']) > 0:
        ax.hist(ti_data['c1'], bins=50, alpha=0.5,
                label=f'C1 (mean={ti_results.get("c1_mean", 0):.1f})', color='blue')
    if len(ti_data['c2']) > 0:
        ax.hist(ti_data['c2'], bins=50, alpha=0.5,
                label=f'C2 (mean={ti_results.get("c2_mean", 0):.1f})', color='red')
    ax.set_xlabel('Tilt Index (dB)')
    ax.set_ylabel('Count')
    ax.set_title(f'Tilt Index: C1 vs C2 (分离度={R["ti_effect"]:.1f} dB)')
    ax.legend()
    ax.grid(True, alpha=0.3)
    plt.tight_layout()
    ti_png = f'{a.out_prefix}_tilt_index.png'
    plt.savefig(ti_png, dpi=150)
    print(f'  TI图已保存: {ti_png}')
    plt.close()


def verify(x, y, sr, *, sr_out=None, frames_in=None, frames_out=None, hyst_db=1.0, up_delay_ms=0,
           target_c2=0.5, fc=1000, slope=12, c1_low=15.0, c1_high=-15.0, c2_low=-15.0,
           c2_high=15.0, n_fft=4096, hop=2048, level_percentile=10, out_prefix='verify_15db_v2',
           plots=True, fused=None):
    """``main()`` of the reference (:539-845) on an input / output pair in memory:
    numpy arrays or resident cuda tensors, [n] or [n, ch].  Prints the reference's
    lines, writes ``<out_prefix>_spectrum.csv``, the two PNGs (``plots``) and
    ``<out_prefix>_report.txt``; returns the results, ``['exit_code']`` 0 or 1.
    ``out_prefix=None`` writes nothing.  ``sr_out`` / ``frames_*``: what the files
    said, where they differ from the arrays."""
    a = argparse.Namespace(hyst_db=hyst_db, up_delay_ms=up_delay_ms, target_c2=target_c2, fc=fc,
                           slope=slope, c1_low=c1_low, c1_high=c1_high, c2_low=c2_low,
                           c2_high=c2_high, n_fft=n_fft, hop=hop,
                           level_percentile=level_percentile, out_prefix=out_prefix)
    fused = FUSED if fused is None else fused
    analysis._check_n_fft(n_fft)
    xd0 = analysis._dev(x, ch=True)
    yd0 = analysis._dev(y, ch=True)

    print('=' * 70)
    print('Tomatis ±15dB 自适应验证工具 v2')
    print('=' * 70)
    print()
    gain_limit = abs(a.c1_low)
    print('滤波器参数:')
    print(f'  fc={a.fc} Hz, slope={a.slope} dB/oct')
    print(f'  C1: +{a.c1_low}/{a.c1_high} dB, C2: {a.c2_low}/+{a.c2_high} dB')
    print(f'  低频封顶: ~{a.fc * 2**(-gain_limit/a.slope):.0f} Hz')
    print(f'  高频封顶: ~{a.fc * 2**(gain_limit/a.slope):.0f} Hz')
    print()
    print('门控参数:')
    print(f'  hyst={a.hyst_db} dB, delay={a.up_delay_ms} ms')
    print(f'  目标 C2 占比: {a.target_c2*100:.0f}%')
    print()

    all_pass = True
    report_lines = ['Tomatis ±15dB 自适应验证报告 v2', '=' * 50]

    # A
    print('-' * 50)
    print('A. 工程检查')
    print('-' * 50)
    eng = _engineering(sr, xd0.shape[1], xd0.shape[0] if frames_in is None else frames_in,
                       sr if sr_out is None else sr_out, yd0.shape[1],
                       yd0.shape[0] if frames_out is None else frames_out, yd0)
    eng_pass = (eng['sr_match'] and eng['ch_match'] and eng['frames_match'] and eng['peak_safe']
                and eng['dc_safe'])
    print(f'  采样率: {eng["sr_in"]} -> {eng["sr_out"]} {"PASS" if eng["sr_match"] else "FAIL"}')
    print(f'  声道数: {eng["ch_in"]} -> {eng["ch_out"]} {"PASS" if eng["ch_match"] else "FAIL"}')
    print(f'  样点数: {eng["frames_in"]} -> {eng["frames_out"]} (diff={eng["frames_diff"]}) '
          f'{"PASS" if eng["frames_match"] else "FAIL"}')
    print(f'  峰值: {eng["peak"]:.4f} ({eng["peak_dbfs"]:.2f} dBFS) '
          f'{"PASS" if eng["peak_safe"] else "FAIL"}')
    print(f'  DC偏移: {eng["dc_mean"]:.6f} {"PASS" if eng["dc_safe"] else "FAIL"}')
    print(f'  结果: {"PASS" if eng_pass else "FAIL"}')
    if not eng_pass:
        all_pass = False
    report_lines.append('\nA. 工程检查')
    report_lines.append(f'  结果: {"PASS" if eng_pass else "FAIL"}')
    report_lines.append(f'  峰值: {eng["peak"]:.4f}')

    # B
    print()
    print('-' * 50)
    print('B. 自适应门控阈值求解')
    print('-' * 50)
    print('  读取输入音频...')
    print('  计算帧电平...')
    levels, _ = analysis.padded_frame_levels(xd0, a.n_fft, a.hop)
    level_median = np.median(levels)
    level_p10 = np.percentile(levels, 10)
    level_p90 = np.percentile(levels, 90)
    print(f'  电平分布: p10={level_p10:.1f}, median={level_median:.1f}, p90={level_p90:.1f} dBFS')
    up_delay_frames = int(a.up_delay_ms * sr / 1000 / a.hop)
    print('  二分查找最优阈值...')
    scan = _scan_of(levels)
    optimal_T, achieved_c2 = _find_optimal_threshold(scan, levels, a.hyst_db, a.target_c2,
                                                     up_delay_frames)
    print(f'  最优阈值 T: {optimal_T:.2f} dBFS')
    print(f'  达成 C2 占比: {achieved_c2*100:.1f}%')
    _, _, codes = scan.run(optimal_T + a.hyst_db / 2, optimal_T - a.hyst_db / 2, up_delay_frames,
                           want_states=True)
    stats = analyze_gate_stats(codes, levels, sr, a.hop)
    c2_ratio_ok = 0.48 <= stats['c2_ratio'] <= 0.52
    print(f'  C2 占比验证 (48%-52%): {"PASS" if c2_ratio_ok else "FAIL"}')
    print(f'  切换次数: {stats["switch_count"]} ({stats["switches_per_min"]:.1f}/min)')
    print(f'  C1/C2 平均电平: {stats["c1_level_mean"]:.1f} / {stats["c2_level_mean"]:.1f} dBFS')
    report_lines.append('\nB. 自适应门控')
    report_lines.append(f'  最优阈值 T: {optimal_T:.2f} dBFS')
    report_lines.append(f'  C2 占比: {achieved_c2*100:.1f}%')
    report_lines.append(f'  切换次数: {stats["switch_count"]}')

    # C (and D's spectra: the same frames of the same pair)
    print()
    print('-' * 50)
    print('C. 条件频谱验证 (改进版)')
    print('-' * 50)
    print(f'  剔除最低 {a.level_percentile}% 能量帧')
    print('  使用 900-1100Hz 频带锚定')
    xd, yd = analysis.pair_on_device(xd0, yd0, a.n_fft // 2)
    anchor = analysis.band_bins(np.fft.rfftfreq(a.n_fft, 1 / sr), 900, 1100)
    rows, be = analysis.verify_spectra(xd, yd, a.n_fft, a.hop, anchor=anchor,
                                       bands=_tilt_bands(sr, a.n_fft), fused=fused)
    F = rows.shape[0]
    freqs, c1_db, c2_db, c1_n, c2_n = _conditional(rows, F, sr, codes, levels, a.n_fft,
                                                   a.level_percentile)
    del rows
    print(f'  有效帧: C1={c1_n}, C2={c2_n}')
    c1_theory = build_tilt_gain_db(freqs, a.fc, a.slope, a.c1_low, a.c1_high)
    c2_theory = build_tilt_gain_db(freqs, a.fc, a.slope, a.c2_low, a.c2_high)
    metrics = compute_spectrum_metrics_v2(freqs, c1_db, c2_db, c1_theory, c2_theory, a.fc,
                                          gain_limit)
    g = metrics.get
    print('  低频平台 (100-350Hz):')
    print(f'    C1: {g("c1_lo_platform_mean", 0):.1f} dB (目标 +{gain_limit}), '
          f'RMSE={g("c1_lo_platform_rmse", 0):.2f}')
    print(f'    C2: {g("c2_lo_platform_mean", 0):.1f} dB (目标 -{gain_limit}), '
          f'RMSE={g("c2_lo_platform_rmse", 0):.2f}')
    print('  高频平台 (3000-10000Hz):')
    print(f'    C1: {g("c1_hi_platform_mean", 0):.1f} dB (目标 -{gain_limit}), '
          f'RMSE={g("c1_hi_platform_rmse", 0):.2f}')
    print(f'    C2: {g("c2_hi_platform_mean", 0):.1f} dB (目标 +{gain_limit}), '
          f'RMSE={g("c2_hi_platform_rmse", 0):.2f}')
    print('  斜坡段 RMSE:')
    print(f'    C1: {g("c1_slope_rmse", 0):.2f} dB, C2: {g("c2_slope_rmse", 0):.2f} dB')
    print('  fc (1000Hz) 误差:')
    print(f'    C1: {g("c1_fc_error", 0):.2f} dB, C2: {g("c2_fc_error", 0):.2f} dB')
    platform_rmse_ok = bool(g('c1_lo_platform_rmse', 99) < 0.5 and g('c2_lo_platform_rmse', 99) < 0.5
                            and g('c1_hi_platform_rmse', 99) < 0.5
                            and g('c2_hi_platform_rmse', 99) < 0.5)
    slope_rmse_ok = bool(g('c1_slope_rmse', 99) < 1.0 and g('c2_slope_rmse', 99) < 1.0)
    fc_ok = bool(g('c1_fc_error', 99) < 0.5 and g('c2_fc_error', 99) < 0.5)
    spectrum_pass = platform_rmse_ok and slope_rmse_ok and fc_ok
    print(f'  平台 RMSE (<0.5dB): {"PASS" if platform_rmse_ok else "FAIL"}')
    print(f'  斜坡 RMSE (<1.0dB): {"PASS" if slope_rmse_ok else "FAIL"}')
    print(f'  fc 误差 (<0.5dB): {"PASS" if fc_ok else "FAIL"}')
    print(f'  条件频谱结果: {"PASS" if spectrum_pass else "FAIL"}')
    if not spectrum_pass:
        all_pass = False
    report_lines.append('\nC. 条件频谱验证')
    report_lines.append(f'  有效帧: C1={c1_n}, C2={c2_n}')
    report_lines.append(f'  平台 RMSE: {"PASS" if platform_rmse_ok else "FAIL"}')
    report_lines.append(f'  斜坡 RMSE: {"PASS" if slope_rmse_ok else "FAIL"}')
    report_lines.append(f'  fc 误差: {"PASS" if fc_ok else "FAIL"}')
    if a.out_prefix is not None:
        csv_path = f'{a.out_prefix}_spectrum.csv'
        with open(csv_path, 'w', newline='', encoding='utf-8') as f:
            writer = csv.writer(f)
            writer.writerow(['freq_hz', 'c1_measured_db', 'c1_theory_db', 'c2_measured_db',
                             'c2_theory_db'])
            for i, freq in enumerate(freqs):
                writer.writerow([f'{freq:.2f}', f'{c1_db[i]:.4f}', f'{c1_theory[i]:.4f}',
                                 f'{c2_db[i]:.4f}', f'{c2_theory[i]:.4f}'])
        print(f'  频谱数据已保存: {csv_path}')

    # D
    print()
    print('-' * 50)
    print('D. 效果量化 (Tilt Index)')
    print('-' * 50)
    ti_data = _tilt(be.cpu().numpy(), F, codes, levels, a.level_percentile)
    ti_results = analyze_tilt_index(ti_data)
    t = ti_results.get
    print(f'  输入 TI (n={t("input_n", 0)}): mean={t("input_mean", 0):.2f}')
    print(f'  输出 TI (n={t("output_n", 0)}): mean={t("output_mean", 0):.2f}')
    print(f'  C1 TI (n={t("c1_n", 0)}): mean={t("c1_mean", 0):.2f}')
    print(f'  C2 TI (n={t("c2_n", 0)}): mean={t("c2_mean", 0):.2f}')
    ti_effect = t('ti_effect', 0)
    print(f'  分离度 (C2-C1): {ti_effect:.2f} dB')
    ti_effect_ok = bool(ti_effect > 20.0)
    print(f'  分离度验证 (>20dB): {"PASS" if ti_effect_ok else f"WARN ({ti_effect:.1f}dB)"}')
    report_lines.append('\nD. 效果量化')
    report_lines.append(f'  C1 TI: {t("c1_mean", 0):.2f} dB')
    report_lines.append(f'  C2 TI: {t("c2_mean", 0):.2f} dB')
    report_lines.append(f'  分离度: {ti_effect:.2f} dB')

    R = dict(eng=eng, eng_pass=eng_pass, levels=levels, optimal_T=optimal_T,
             achieved_c2=achieved_c2, codes=codes, stats=stats, c2_ratio_ok=c2_ratio_ok,
             freqs=freqs, c1_db=c1_db, c2_db=c2_db, c1_n=c1_n, c2_n=c2_n, c1_theory=c1_theory,
             c2_theory=c2_theory, metrics=metrics, platform_rmse_ok=platform_rmse_ok,
             slope_rmse_ok=slope_rmse_ok, fc_ok=fc_ok, spectrum_pass=spectrum_pass,
             ti_data=ti_data, ti=ti_results, ti_effect=ti_effect, ti_effect_ok=ti_effect_ok,
             gain_limit=gain_limit)
    if plots and a.out_prefix is not None:
        _plots(a, R)

    print()
    print('=' * 70)
    print('最终判定')
    print('=' * 70)
    print(f'  A. 工程检查: {"PASS" if eng_pass else "FAIL"}')
    print(f'  B. 门控 C2 占比 ({achieved_c2*100:.0f}%): {"PASS" if c2_ratio_ok else "FAIL"}')
    print(f'  C. 条件频谱: {"PASS" if spectrum_pass else "FAIL"}')
    print(f'  D. TI 分离度 ({ti_effect:.0f}dB): {"PASS" if ti_effect_ok else "WARN"}')
    print()
    ok = bool(all_pass and c2_ratio_ok)
    if ok:
        print('验证结果: PASS')
        print('D_MNF_matched_15dB.flac 符合 Tomatis ±15dB 规则')
    else:
        print('验证结果: FAIL')
        print('请检查上述 FAIL 项')
    report_lines.append('\n' + '=' * 50)
    report_lines.append(f'总体结果: {"PASS" if ok else "FAIL"}')
    R['report'] = '\n'.join(report_lines)
    if a.out_prefix is not None:
        report_path = f'{a.out_prefix}_report.txt'
        with open(report_path, 'w', encoding='utf-8') as f:
            f.write(R['report'])
        print(f'\n报告已保存: {report_path}')
    R['exit_code'] = 0 if ok else 1
    return R


def build_parser():
    parser = argparse.ArgumentParser(description='Tomatis ±15dB 自适应验证工具 v2')
    parser.add_argument('-i', '--input', required=True, help='原始输入音频')
    parser.add_argument('-o', '--output', required=True, help='处理后输出音频')
    parser.add_argument('--hyst_db', type=float, default=1.0, help='回差 dB')
    parser.add_argument('--up_delay_ms', type=float, default=0, help='上行延迟 ms')
    parser.add_argument('--target_c2', type=float, default=0.5, help='目标 C2 占比')
    parser.add_argument('--fc', type=float, default=1000)
    parser.add_argument('--slope', type=float, default=12)
    parser.add_argument('--c1_low', type=float, default=15.0)
    parser.add_argument('--c1_high', type=float, default=-15.0)
    parser.add_argument('--c2_low', type=float, default=-15.0)
    parser.add_argument('--c2_high', type=float, default=15.0)
    parser.add_argument('--n_fft', type=int, default=4096)
    parser.add_argument('--hop', type=int, default=2048)
    parser.add_argument('--level_percentile', type=float, default=10, help='剔除最低 N%% 能量帧')
    parser.add_argument('--out_prefix', default='verify_15db_v2')
    return parser


def main(argv=None):
    """verify_tomatis_15db_v2.py:509-845; returns 0 (PASS) or 1 (FAIL)."""
    args = build_parser().parse_args(argv)
    sr_in, ch_in, n_in = audio_io.info(args.input)
    sr_out, ch_out, n_out = audio_io.info(args.output)
    x, sr = audio_io.read(args.input)
    y, _ = audio_io.read(args.output)
    kw = {k: v for k, v in vars(args).items() if k not in ('input', 'output')}
    return verify(x, y, sr, sr_out=sr_out, frames_in=n_in, frames_out=n_out, **kw)['exit_code']


__all__ = ['rms_dbfs', 'build_tilt_gain_db', 'check_engineering', 'compute_frame_levels',
           'simulate_gate_with_threshold', 'find_optimal_threshold', 'analyze_gate_stats',
           'find_stable_frames', 'compute_conditional_spectrum_v2',
           'compute_spectrum_metrics_v2', 'compute_tilt_index', 'analyze_tilt_index', 'verify',
           'main']


if __name__ == '__main__':
    sys.exit(main())
