"""Layer-1 acceptance validator — MI355X drop-in for src/validate_layer1.py
(SURVEY.md §8 row f9): judges a processed file against the state CSV that
``process_tomatis --state_csv`` wrote.  It checks that the implementation follows
its parameters (gate logic, filter shape, engineering integrity), not that it
matches any hardware.

Same function names, flags, defaults, printed lines, CSV header and number
formats and PNG as the reference; the PCM is uploaded once and everything per
sample or per bin runs in ``libtomatis_hip.so``:

  reference (file:line)              here
  ---------------------------------- --------------------------------------------
  check_engineering :62-88           audio_io.info; tomatis_absmax (peak)
  load_state_csv :95-107             host (a text file)
  simulate_gate :110-163             zero padding on the device, tomatis_an_frame_r
                                     (bit-exact r), the reference's
                                     ``20 log10(r + EPS)`` on the host, then
                                     tomatis_cal_gate_grid with the padded frame
                                     starts and the up-delay in samples
  compare_gate_states :166-193,      host: numpy on per-frame lists
  analyze_gate_stats :200-238
  compute_conditional_spectrum       analysis.compute_conditional_spectrum
  :261-389                           (tm_analysis.hip), unchanged
  compute_spectrum_rmse :392-398     host: bins

``validate(x, y, sr, csv_frames, ...)`` is ``main()`` minus argparse and the
file reads.  There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import csv
import sys

import numpy as np

from . import analysis, audio_io
from .analysis import compute_conditional_spectrum, find_stable_frames  # noqa: F401
from .dsp import build_tilt_gain_db  # noqa: F401  (reference name, :41-55)

EPS = 1e-12


def rms_dbfs(x_mono: np.ndarray) -> float:
    """validate_layer1.py:35-38 (host, one frame)."""
    r = np.sqrt(np.mean(x_mono * x_mono) + EPS)
    return float(20.0 * np.log10(r + EPS))


def _engineering(sr_in, ch_in, frames_in, sr_out, ch_out, frames_out, yd):
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
    return results


def check_engineering(in_path, out_path):
    """:62-88: sample rate / channels / length / peak of two files."""
    sr_in, ch_in, n_in = audio_io.info(in_path)
    sr_out, ch_out, n_out = audio_io.info(out_path)
    y, _ = audio_io.read(out_path)
    return _engineering(sr_in, ch_in, n_in, sr_out, ch_out, n_out, analysis._dev(y, ch=True))


def load_state_csv(csv_path):
    """:95-107."""
    frames = []
    with open(csv_path, 'r', encoding='utf-8') as f:
        for row in csv.DictReader(f):
            frames.append({'frame_idx': int(row['frame_idx']),
                           'time_sec': float(row['time_sec']),
                           'level_dbfs': float(row['level_dbfs']),
                           'state': row['state']})
    return frames


def _simulate_gate(xd, sr, n_fft, hop, threshold_dbfs, hyst_db, up_delay_ms):
    """-> (int8 codes, float64 levels)."""
    Ton = threshold_dbfs + hyst_db / 2
    Toff = threshold_dbfs - hyst_db / 2
    up_delay_samples = int(up_delay_ms * sr / 1000)
    levels, starts = analysis.padded_frame_levels(xd, n_fft, hop)
    _, _, codes = analysis.GateScan(levels, starts).run(Ton, Toff, up_delay_samples,
                                                        want_states=True)
    return codes, levels


def simulate_gate(x, sr, n_fft, hop, threshold_dbfs, hyst_db, up_delay_ms):
    """:110-163: the gate re-computed from the input -> (states, levels) lists."""
    codes, levels = _simulate_gate(analysis._dev(x, ch=True), sr, n_fft, hop, threshold_dbfs,
                                   hyst_db, up_delay_ms)
    return analysis.state_names(codes), levels.tolist()


def _switches(codes):
    return int(np.count_nonzero(codes[1:] != codes[:-1])) if len(codes) > 1 else 0


def compare_gate_states(csv_states, sim_states, sim_levels, csv_levels):
    """:166-193."""
    a, b = analysis.state_codes(csv_states), analysis.state_codes(sim_states)
    n = min(len(a), len(b))
    mismatch_count = int(np.count_nonzero(a[:n] != b[:n]))
    level_diffs = np.abs(np.asarray(csv_levels, np.float64)[:n]
                         - np.asarray(sim_levels, np.float64)[:n])
    csv_switches, sim_switches = _switches(a), _switches(b)
    return {
        'total_frames': n,
        'mismatch_count': mismatch_count,
        'mismatch_rate': mismatch_count / n if n > 0 else 0,
        'csv_switches': csv_switches,
        'sim_switches': sim_switches,
        'switch_diff': abs(csv_switches - sim_switches),
        'level_max_diff': float(level_diffs.max()) if n > 0 else 0,
        'level_mean_diff': np.mean(level_diffs) if n > 0 else 0,
    }


def analyze_gate_stats(states):
    """:200-238."""
    codes = analysis.state_codes(states)
    n = len(codes)
    if n == 0:
        return {}
    c2_count = int(np.count_nonzero(codes == 2))
    cut = np.nonzero(codes[1:] != codes[:-1])[0] + 1
    run_lengths = np.diff(np.concatenate([[0], cut, [n]]))
    short_runs = int(np.count_nonzero(run_lengths <= 3))
    return {
        'total_frames': n,
        'c2_count': c2_count,
        'c2_ratio': c2_count / n,
        'switch_count': len(run_lengths) - 1,
        'run_count': len(run_lengths),
        'run_min': int(run_lengths.min()),
        'run_max': int(run_lengths.max()),
        'run_median': np.median(run_lengths),
        'short_runs': short_runs,
        'short_run_ratio': short_runs / len(run_lengths),
    }


def compute_spectrum_rmse(measured_db, theory_db, freqs, f_low, f_high):
    """:392-398."""
    mask = (freqs >= f_low) & (freqs <= f_high)
    if not np.any(mask):
        return 0.0
    diff = measured_db[mask] - theory_db[mask]
    return np.sqrt(np.mean(diff ** 2))


def _plot(a, freqs, c1_db, c1_theory, c2_db, c2_theory, c1_n, c2_n):
    """:614-652."""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        print('matplotlib 未安装，跳过绘图')
        return
    fig, axes = plt.subplots(2, 1, figsize=(12, 8))
    for ax, name, col, meas, th, n_used in ((axes[0], 'C1', 'b', c1_db, c1_theory, c1_n),
                                            (axes[1], 'C2', 'r', c2_db, c2_theory, c2_n)):
        ax.semilogx(freqs, meas, col + '-', label=f'{name} measured', alpha=0.7)
        ax.semilogx(freqs, th, col + '--', label=f'{name} theory', linewidth=2)
        ax.axhline(0, color='gray', linestyle=':')
        ax.axvline(a.fc, color='red', linestyle=':', label=f'fc={a.fc}Hz')
        ax.set_xlim(20, 20000)
        ax.set_ylim(-10, 10)
        ax.set_xlabel('Frequency (Hz)')
        ax.set_ylabel('Gain (dB)')
        ax.set_title(f'{name} Spectrum (n={n_used})')
        ax.legend()
        ax.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(a.out_png, dpi=150)
    print(f'频谱图已保存: {a.out_png}')
    plt.close()


def validate(x, y, sr, csv_frames, *, sr_out=None, frames_in=None, frames_out=None, gate_ui=50,
             gate_scale=1.0, gate_offset=-61.08, hyst_db=1.0, up_delay_ms=0, fc=1000, slope=12,
             c1_low=5.0, c1_high=-5.0, c2_low=-5.0, c2_high=5.0, n_fft=4096, hop=2048,
             out_csv='layer1_spectrum_check.csv', out_png='layer1_spectrum_check.png'):
    """``main()`` of the reference (:436-679) on an input / output pair in memory
    (numpy arrays or resident cuda tensors) and the rows of the state CSV; prints
    the reference's lines, writes ``out_csv`` and ``out_png`` (None: not written);
    returns the results, ``['exit_code']`` 0 or 1."""
    a = argparse.Namespace(gate_ui=gate_ui, gate_scale=gate_scale, gate_offset=gate_offset,
                           hyst_db=hyst_db, up_delay_ms=up_delay_ms, fc=fc, slope=slope,
                           c1_low=c1_low, c1_high=c1_high, c2_low=c2_low, c2_high=c2_high,
                           n_fft=n_fft, hop=hop, out_csv=out_csv, out_png=out_png)
    analysis._check_n_fft(n_fft)
    xd = analysis._dev(x, ch=True)
    yd = analysis._dev(y, ch=True)
    print('=' * 60)
    print('Layer1 验证工具')
    print('=' * 60)
    print()
    print('验证目标: 算法实现是否符合参数设定')
    print('  - 门控逻辑: RMS dBFS + 回差 + 延迟')
    print('  - 滤波形状: fc/slope/gain')
    print('  - 工程完整性: 长度、削波')
    print('注意: 本工具不验证"与硬件一模一样"')
    print()
    threshold_dbfs = a.gate_scale * a.gate_ui + a.gate_offset
    print('参数:')
    print(f'  Gate: UI={a.gate_ui}, T={threshold_dbfs:.2f} dBFS, hyst={a.hyst_db} dB, '
          f'delay={a.up_delay_ms} ms')
    print(f'  Filter: fc={a.fc} Hz, slope={a.slope} dB/oct')
    print(f'  C1: low={a.c1_low} dB, high={a.c1_high} dB')
    print(f'  C2: low={a.c2_low} dB, high={a.c2_high} dB')
    print()
    results = {'pass': True, 'checks': {}}

    print('-' * 40)
    print('A. 工程检查')
    print('-' * 40)
    eng = _engineering(sr, xd.shape[1], xd.shape[0] if frames_in is None else frames_in,
                       sr if sr_out is None else sr_out, yd.shape[1],
                       yd.shape[0] if frames_out is None else frames_out, yd)
    print(f'  采样率: {eng["sr_in"]} -> {eng["sr_out"]} {"PASS" if eng["sr_match"] else "FAIL"}')
    print(f'  声道数: {eng["ch_in"]} -> {eng["ch_out"]} {"PASS" if eng["ch_match"] else "FAIL"}')
    print(f'  样点数: {eng["frames_in"]} -> {eng["frames_out"]} (diff={eng["frames_diff"]}) '
          f'{"PASS" if eng["frames_match"] else "FAIL"}')
    print(f'  峰值: {eng["peak"]:.4f} {"PASS" if eng["peak_safe"] else "FAIL (>=0.98)"}')
    results['checks']['engineering'] = {k: eng[k] for k in ('sr_match', 'ch_match',
                                                            'frames_match', 'peak_safe')}
    if not all(results['checks']['engineering'].values()):
        results['pass'] = False

    print()
    print('-' * 40)
    print('B. Gate 独立复算')
    print('-' * 40)
    csv_states = [f['state'] for f in csv_frames]
    csv_levels = [f['level_dbfs'] for f in csv_frames]
    sim_codes, sim_levels = _simulate_gate(xd, sr, a.n_fft, a.hop, threshold_dbfs, a.hyst_db,
                                           a.up_delay_ms)
    cmp = compare_gate_states(csv_states, sim_codes, sim_levels, csv_levels)
    print(f'  总帧数: {cmp["total_frames"]}')
    print(f'  状态不匹配: {cmp["mismatch_count"]} ({cmp["mismatch_rate"]*100:.2f}%)')
    print(f'  切换次数: CSV={cmp["csv_switches"]}, SIM={cmp["sim_switches"]}, '
          f'diff={cmp["switch_diff"]}')
    print(f'  电平最大差: {cmp["level_max_diff"]:.4f} dB')
    print(f'  电平平均差: {cmp["level_mean_diff"]:.4f} dB')
    gate_ok = bool(cmp['mismatch_rate'] < 0.01 and cmp['level_max_diff'] < 0.1)
    print(f'  结果: {"PASS" if gate_ok else "FAIL (mismatch>1% or level_diff>0.1dB)"}')
    results['checks']['gate_verify'] = {'mismatch_rate': cmp['mismatch_rate'],
                                        'level_max_diff': cmp['level_max_diff'], 'pass': gate_ok}
    results['sim_codes'], results['sim_levels'], results['cmp'] = sim_codes, sim_levels, cmp
    if not gate_ok:
        results['pass'] = False

    print()
    print('-' * 40)
    print('C. Gate 统计')
    print('-' * 40)
    stats = analyze_gate_stats(csv_states)
    duration_min = stats['total_frames'] * a.hop / sr / 60
    switches_per_min = stats['switch_count'] / duration_min if duration_min > 0 else 0
    print(f'  C2 占比: {stats["c2_ratio"]*100:.1f}%')
    print(f'  切换次数: {stats["switch_count"]} (约 {switches_per_min:.1f}/min)')
    print(f'  Run length: min={stats["run_min"]}, max={stats["run_max"]}, '
          f'median={stats["run_median"]:.0f}')
    print(f'  短段(<=3帧): {stats["short_runs"]} ({stats["short_run_ratio"]*100:.1f}%)')
    c2_ratio_ok = 0.05 <= stats['c2_ratio'] <= 0.95
    jitter_ok = stats['short_run_ratio'] < 0.3
    print(f'  C2占比范围: {"PASS" if c2_ratio_ok else "WARN (极端值)"}')
    print(f'  抖动检测: {"PASS" if jitter_ok else "WARN (短段过多)"}')
    results['checks']['gate_stats'] = {'c2_ratio': stats['c2_ratio'],
                                       'short_run_ratio': stats['short_run_ratio'],
                                       'c2_ratio_ok': c2_ratio_ok, 'jitter_ok': jitter_ok}
    results['stats'] = stats

    print()
    print('-' * 40)
    print('D. 条件频谱验证')
    print('-' * 40)
    xs, ys = analysis.pair_on_device(xd, yd, a.n_fft // 2)
    freqs, c1_db, c2_db, c1_n, c2_n = compute_conditional_spectrum(
        xs, ys, sr, csv_states, a.n_fft, a.hop, level_threshold=-60)
    print(f'  稳定帧: C1={c1_n}, C2={c2_n}')
    c1_theory = build_tilt_gain_db(freqs, a.fc, a.slope, a.c1_low, a.c1_high)
    c2_theory = build_tilt_gain_db(freqs, a.fc, a.slope, a.c2_low, a.c2_high)
    bands = [('low', 100, 800), ('mid', 800, 1200), ('high', 2000, 8000)]
    print('  C1 RMSE:')
    c1_rmse_all = []
    for name, f_low, f_high in bands:
        rmse = compute_spectrum_rmse(c1_db, c1_theory, freqs, f_low, f_high)
        c1_rmse_all.append(rmse)
        print(f'    {name} ({f_low}-{f_high}Hz): {rmse:.2f} dB')
    print('  C2 RMSE:')
    c2_rmse_all = []
    for name, f_low, f_high in bands:
        rmse = compute_spectrum_rmse(c2_db, c2_theory, freqs, f_low, f_high)
        c2_rmse_all.append(rmse)
        print(f'    {name} ({f_low}-{f_high}Hz): {rmse:.2f} dB')
    spectrum_ok = bool(max(c1_rmse_all + c2_rmse_all) < 1.5)
    print(f'  结果: {"PASS" if spectrum_ok else "FAIL (RMSE >= 1.5 dB)"}')
    results['checks']['spectrum'] = {'c1_rmse': c1_rmse_all, 'c2_rmse': c2_rmse_all,
                                     'pass': spectrum_ok}
    results.update(freqs=freqs, c1_db=c1_db, c2_db=c2_db, c1_n=c1_n, c2_n=c2_n,
                   c1_theory=c1_theory, c2_theory=c2_theory, eng=eng)
    if not spectrum_ok:
        results['pass'] = False

    if a.out_csv is not None:
        with open(a.out_csv, 'w', newline='', encoding='utf-8') as f:
            writer = csv.writer(f)
            writer.writerow(['freq_hz', 'c1_measured_db', 'c1_theory_db', 'c2_measured_db',
                             'c2_theory_db'])
            for i, freq in enumerate(freqs):
                writer.writerow([f'{freq:.2f}', f'{c1_db[i]:.4f}', f'{c1_theory[i]:.4f}',
                                 f'{c2_db[i]:.4f}', f'{c2_theory[i]:.4f}'])
        print(f'\n频谱数据已保存: {a.out_csv}')
    if a.out_png is not None:
        _plot(a, freqs, c1_db, c1_theory, c2_db, c2_theory, c1_n, c2_n)

    print()
    print('=' * 60)
    print('最终判定')
    print('=' * 60)
    all_checks = [('工程检查', all(results['checks']['engineering'].values())),
                  ('Gate复算', results['checks']['gate_verify']['pass']),
                  ('条件频谱', results['checks']['spectrum']['pass'])]
    for name, passed in all_checks:
        print(f'  {name}: {"PASS" if passed else "FAIL"}')
    print()
    if results['pass']:
        print('Layer1 验证: PASS')
        print('算法实现符合参数设定')
    else:
        print('Layer1 验证: FAIL')
        print('请检查上述 FAIL 项')
    results['exit_code'] = 0 if results['pass'] else 1
    return results


def build_parser():
    parser = argparse.ArgumentParser(description='Layer1 验证工具')
    parser.add_argument('-i', '--input', required=True, help='原始输入音频')
    parser.add_argument('-o', '--output', required=True, help='Layer1 输出音频')
    parser.add_argument('--state_csv', required=True, help='状态 CSV 文件')
    parser.add_argument('--gate_ui', type=float, default=50)
    parser.add_argument('--gate_scale', type=float, default=1.0)
    parser.add_argument('--gate_offset', type=float, default=-61.08)
    parser.add_argument('--hyst_db', type=float, default=1.0)
    parser.add_argument('--up_delay_ms', type=float, default=0)
    parser.add_argument('--fc', type=float, default=1000)
    parser.add_argument('--slope', type=float, default=12)
    parser.add_argument('--c1_low', type=float, default=5.0)
    parser.add_argument('--c1_high', type=float, default=-5.0)
    parser.add_argument('--c2_low', type=float, default=-5.0)
    parser.add_argument('--c2_high', type=float, default=5.0)
    parser.add_argument('--n_fft', type=int, default=4096)
    parser.add_argument('--hop', type=int, default=2048)
    parser.add_argument('--out_csv', default='layer1_spectrum_check.csv')
    parser.add_argument('--out_png', default='layer1_spectrum_check.png')
    return parser


def main(argv=None):
    """validate_layer1.py:405-679; returns 0 (PASS) or 1 (FAIL)."""
    args = build_parser().parse_args(argv)
    sr_in, ch_in, n_in = audio_io.info(args.input)
    sr_out, ch_out, n_out = audio_io.info(args.output)
    x, sr = audio_io.read(args.input)
    y, _ = audio_io.read(args.output)
    kw = {k: v for k, v in vars(args).items() if k not in ('input', 'output', 'state_csv')}
    return validate(x, y, sr, load_state_csv(args.state_csv), sr_out=sr_out, frames_in=n_in,
                    frames_out=n_out, **kw)['exit_code']


__all__ = ['rms_dbfs', 'build_tilt_gain_db', 'check_engineering', 'load_state_csv',
           'simulate_gate', 'compare_gate_states', 'analyze_gate_stats', 'find_stable_frames',
           'compute_conditional_spectrum', 'compute_spectrum_rmse', 'validate', 'main']


if __name__ == '__main__':
    sys.exit(main())
