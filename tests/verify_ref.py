"""numpy statement of the two acceptance validators' arithmetic
(src/validate_layer1.py, src/verify_tomatis_15db_v2.py), written from their
description: float32 as the reference runs it (``dtype=np.float32``), or the same
formulas in float64 on the same float32 samples and window (``np.float64``), which
the device's error is measured against.  tools/make_verify_goldens.py checks that
the float32 statement reproduces the reference's CSV columns, counts and report."""
from __future__ import annotations

import hashlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

EPS = 1e-12


def _2d(a, dtype=None):
    a = np.asarray(a)
    a = a.reshape(len(a), -1)
    return a if dtype is None else a.astype(dtype)


def tilt_gain_db(freqs, fc, slope, low_db, high_db):
    f = np.maximum(freqs, 1.0)
    o = np.log2(f / fc).astype(np.float32)
    g = np.zeros_like(o, dtype=np.float32)
    lo = np.sign(low_db) * np.minimum(slope * np.maximum(0.0, -o), abs(low_db))
    hi = np.sign(high_db) * np.minimum(slope * np.maximum(0.0, o), abs(high_db))
    g[o < 0] = lo[o < 0]
    g[o > 0] = hi[o > 0]
    return g


# ---------------------------------------------------------------------------
# levels and gate
# ---------------------------------------------------------------------------

def frame_levels(x, n_fft, hop):
    """The padded level grid -> (levels float64 of float32 values, padded starts)."""
    x = _2d(x, np.float32)
    n, ch = x.shape
    pad = n_fft // 2
    z = np.zeros((pad, ch), np.float32)
    xp = np.vstack([z, x, z])
    mono = np.sqrt(np.mean(xp ** 2, axis=1))
    m2 = mono * mono
    starts = np.arange(0, len(xp) - n_fft + 1, hop, dtype=np.int64)
    starts = starts[(starts - pad >= 0) & (starts - pad < n)]
    lv = np.empty(len(starts), np.float64)
    win = sliding_window_view(m2, n_fft)
    for a in range(0, len(starts), 256):
        fr = np.ascontiguousarray(win[starts[a:a + 256]])
        r = np.sqrt(np.mean(fr, axis=1) + EPS)          # float32
        lv[a:a + 256] = 20.0 * np.log10(r + EPS)
    return lv, starts


def gate(levels, starts, Ton, Toff, up_delay):
    """The validators' automaton, sequentially -> int8 codes (1 / 2)."""
    out = np.empty(len(levels), np.int8)
    state, pending = 1, None
    for i, (lv, s) in enumerate(zip(np.asarray(levels).tolist(), np.asarray(starts).tolist())):
        if state == 1:
            if lv >= Ton:
                if pending is None:
                    pending = s + up_delay
            else:
                pending = None
            if pending is not None and s >= pending:
                state, pending = 2, None
        elif lv <= Toff:
            state, pending = 1, None
        out[i] = state
    return out


def gate_frames(levels, T, hyst, up_delay_frames=0):
    return gate(levels, np.arange(len(levels)), T + hyst / 2, T - hyst / 2, up_delay_frames)


def find_optimal_threshold(levels, hyst, target=0.5, up_delay_frames=0):
    lo, hi = np.min(levels) - 10, np.max(levels) + 10
    best_T, best_ratio, best_diff = np.median(levels), 0.0, 1.0
    for _ in range(30):
        mid = (lo + hi) / 2
        ratio = int(np.count_nonzero(gate_frames(levels, mid, hyst, up_delay_frames) == 2)) \
            / len(levels)
        diff = abs(ratio - target)
        if diff < best_diff:
            best_diff, best_T, best_ratio = diff, mid, ratio
        if diff < 0.01:
            break
        if ratio < target:
            hi = mid
        else:
            lo = mid
    return best_T, best_ratio


def switches(codes):
    return int(np.count_nonzero(codes[1:] != codes[:-1])) if len(codes) > 1 else 0


def run_lengths(codes):
    cut = np.nonzero(codes[1:] != codes[:-1])[0] + 1
    return np.diff(np.concatenate([[0], cut, [len(codes)]]))


def state_sha(codes):
    return hashlib.sha256("".join("C%d" % v for v in np.asarray(codes).tolist())
                          .encode()).hexdigest()


def stable(codes, margin=2):
    """-> (stable C1 indices, stable C2 indices)."""
    n = len(codes)
    c1, c2 = [], []
    for i in range(margin, n - margin):
        w = codes[i - margin:i + margin + 1]
        if np.all(w == 1):
            c1.append(i)
        elif np.all(w == 2):
            c2.append(i)
    return np.asarray(c1, np.int64), np.asarray(c2, np.int64)


# ---------------------------------------------------------------------------
# spectra of the frames fully inside x
# ---------------------------------------------------------------------------

def _pair(x, y, n_fft, dtype):
    x, y = _2d(x, dtype), _2d(y, dtype)
    if len(y) < len(x):
        assert len(x) - len(y) <= n_fft // 2
        y = np.vstack([y, np.zeros((len(x) - len(y), y.shape[1]), dtype)])
    return x, y[:len(x)]


def _mags(x, n_fft, hop, idx, dtype, power=False):
    """mean over channels of |rfft(win * frame)| (or its square) for frames idx."""
    win = np.hanning(n_fft).astype(np.float32).astype(dtype)
    nb = n_fft // 2 + 1
    out = np.zeros((len(idx), nb), dtype)
    for c in range(x.shape[1]):
        fr = sliding_window_view(x[:, c], n_fft)[np.asarray(idx, np.int64) * hop]
        m = np.abs(np.fft.rfft(fr * win, axis=1))
        out += m ** 2 if power else m
    out /= x.shape[1]
    return out


def n_inside(n, n_fft, hop):
    return max(0, 1 + (n - n_fft) // hop)


def ratio_rows(x, y, n_fft, hop, a0, a1, dtype=np.float32, idx=None):
    """-> (anchored rows, mean_c|X_c|, mean_c|Y_c|) of frames idx (default: all)."""
    x, y = _pair(x, y, n_fft, dtype)
    idx = np.arange(n_inside(len(x), n_fft, hop)) if idx is None else idx
    X = _mags(x, n_fft, hop, idx, dtype)
    Y = _mags(y, n_fft, hop, idx, dtype)
    ratio = Y / np.maximum(X, dtype(1e-10))
    if a1 > a0:
        g = np.mean(ratio[:, a0:a1], axis=1)
        ok = g > 0
        ratio[ok] = ratio[ok] / g[ok, None]
    return ratio, X, Y


def band_energies(x, y, n_fft, hop, lo0, lo1, hi0, hi1, dtype=np.float32, idx=None):
    """-> [F, 4]: sum P_x[lo), sum P_x[hi), sum P_y[lo), sum P_y[hi)."""
    x, y = _pair(x, y, n_fft, dtype)
    idx = np.arange(n_inside(len(x), n_fft, hop)) if idx is None else idx
    PX = _mags(x, n_fft, hop, idx, dtype, power=True)
    PY = _mags(y, n_fft, hop, idx, dtype, power=True)
    return np.stack([PX[:, lo0:lo1].sum(axis=1), PX[:, hi0:hi1].sum(axis=1),
                     PY[:, lo0:lo1].sum(axis=1), PY[:, hi0:hi1].sum(axis=1)], axis=1)


def band_bins(freqs, f_lo, f_hi):
    idx = np.nonzero((freqs >= f_lo) & (freqs <= f_hi))[0]
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def conditional_v2(x, y, sr, codes, levels, n_fft, hop, pct=10, anchor=(900, 1100),
                   dtype=np.float32):
    """-> (freqs, c1_db, c2_db, c1_used, c2_used)."""
    x2 = _2d(x)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    a0, a1 = band_bins(freqs, *anchor)
    thr = np.percentile(levels, pct)
    F = n_inside(len(x2), n_fft, hop)
    out, used = [], []
    for idx in stable(codes):
        idx = idx[(idx < F)]
        idx = idx[~(np.asarray(levels)[idx] < thr)]
        used.append(len(idx))
        if len(idx):
            rows, _, _ = ratio_rows(x, y, n_fft, hop, a0, a1, dtype, idx)
            out.append(20 * np.log10(np.median(rows, axis=0) + EPS))
        else:
            out.append(np.zeros(len(freqs)))
    return freqs, out[0], out[1], used[0], used[1]


def conditional_l1(x, y, sr, codes, n_fft, hop, level_threshold=-60, dtype=np.float32):
    """validate_layer1's conditional spectrum: un-anchored, frames at or above
    level_threshold (their own un-padded level)."""
    x2 = _2d(x, np.float32)
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    F = n_inside(len(x2), n_fft, hop)
    mono = np.sqrt(np.mean(x2 ** 2, axis=1))
    m2 = mono * mono
    out, used = [], []
    for idx in stable(codes):
        idx = idx[idx < F]
        if len(idx):
            fr = np.ascontiguousarray(sliding_window_view(m2, n_fft)[idx * hop])
            r = np.sqrt(np.mean(fr, axis=1) + EPS)
            lv = (20.0 * np.log10(r + EPS)).astype(np.float64)
            idx = idx[~(lv < level_threshold)]
        used.append(len(idx))
        if len(idx):
            rows, _, _ = ratio_rows(x, y, n_fft, hop, 0, 0, dtype, idx)
            out.append(20 * np.log10(np.median(rows, axis=0) + EPS))
        else:
            out.append(np.zeros(len(freqs)))
    return freqs, out[0], out[1], used[0], used[1]


def metrics_v2(freqs, c1_db, c2_db, th1, th2, fc, gain_limit):
    m = {}
    f_lo, f_hi = fc * 2 ** (-gain_limit / 12), fc * 2 ** (gain_limit / 12)

    def rmse(a, b, k):
        return np.sqrt(np.mean((a[k] - b[k]) ** 2))

    for key, k in (("lo_platform", (freqs >= 100) & (freqs <= f_lo * 0.8)),
                   ("hi_platform", (freqs >= f_hi * 1.2) & (freqs <= 10000))):
        if np.any(k):
            m[f"c1_{key}_rmse"], m[f"c2_{key}_rmse"] = rmse(c1_db, th1, k), rmse(c2_db, th2, k)
            m[f"c1_{key}_mean"], m[f"c2_{key}_mean"] = np.mean(c1_db[k]), np.mean(c2_db[k])
    k = (freqs >= f_lo * 1.2) & (freqs <= f_hi * 0.8)
    if np.any(k):
        m["c1_slope_rmse"], m["c2_slope_rmse"] = rmse(c1_db, th1, k), rmse(c2_db, th2, k)
    k = (freqs >= 900) & (freqs <= 1100)
    if np.any(k):
        m["c1_fc_error"], m["c2_fc_error"] = abs(np.mean(c1_db[k])), abs(np.mean(c2_db[k]))
    return m


def tilt_index(x, y, sr, codes, levels, n_fft, hop, pct=10, dtype=np.float32):
    """-> dict input / output / c1 / c2 of tilt indices."""
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    lo, hi = band_bins(freqs, 200, 1000), band_bins(freqs, 2000, 8000)
    F = min(n_inside(len(_2d(x)), n_fft, hop), len(codes))
    thr = np.percentile(levels, pct)
    idx = np.nonzero(~(np.asarray(levels)[:F] < thr))[0]
    e = band_energies(x, y, n_fft, hop, *lo, *hi, dtype, idx)
    c = np.asarray(codes)[idx]
    eps = dtype(EPS)
    okx, oky = e[:, 0] > eps, e[:, 2] > eps
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = 10 * np.log10(e[:, 1] / e[:, 0] + eps)
        ty = 10 * np.log10(e[:, 3] / e[:, 2] + eps)
    return dict(input=tx[okx], output=ty[oky], c1=ty[oky & (c == 1)], c2=ty[oky & (c != 1)])


def tilt_stats(ti):
    r = {}
    for k in ("input", "output", "c1", "c2"):
        if len(ti[k]):
            r[k + "_mean"], r[k + "_std"], r[k + "_n"] = np.mean(ti[k]), np.std(ti[k]), len(ti[k])
    if "c1_mean" in r and "c2_mean" in r:
        r["ti_effect"] = r["c2_mean"] - r["c1_mean"]
    return r


# ---------------------------------------------------------------------------
# the two validators end to end
# ---------------------------------------------------------------------------

def run_v2(x, y, sr, a, frames_in=None, frames_out=None, dtype=np.float32):
    """verify_tomatis_15db_v2 on arrays with the argument dict ``a``."""
    x2, y2 = _2d(x, np.float32), _2d(y, np.float32)
    n_in = len(x2) if frames_in is None else frames_in
    n_out = len(y2) if frames_out is None else frames_out
    R = {}
    peak = np.max(np.abs(y2)) if y2.size else np.float32(0)
    R["peak"] = np.float32(peak)
    R["dc"] = float(np.mean(y2.astype(np.float64))) if y2.size else 0.0
    R["dc32"] = np.mean(y2) if y2.size else np.float32(0)
    R["eng_pass"] = bool(x2.shape[1] == y2.shape[1] and n_in == n_out and peak < 0.98
                         and abs(R["dc32"]) < 0.001)
    levels, _ = frame_levels(x2, a["n_fft"], a["hop"])
    udf = int(a["up_delay_ms"] * sr / 1000 / a["hop"])
    T, ratio = find_optimal_threshold(levels, a["hyst_db"], a["target_c2"], udf)
    codes = gate_frames(levels, T, a["hyst_db"], udf)
    R.update(levels=levels, T=T, ratio=ratio, codes=codes, switch_count=switches(codes),
             c2_ratio=int(np.count_nonzero(codes == 2)) / len(codes))
    R["c2_ratio_ok"] = bool(0.48 <= R["c2_ratio"] <= 0.52)
    freqs, c1, c2, n1, n2 = conditional_v2(x2, y2, sr, codes, levels, a["n_fft"], a["hop"],
                                           a["level_percentile"], dtype=dtype)
    th1 = tilt_gain_db(freqs, a["fc"], a["slope"], a["c1_low"], a["c1_high"])
    th2 = tilt_gain_db(freqs, a["fc"], a["slope"], a["c2_low"], a["c2_high"])
    gl = abs(a["c1_low"])
    m = metrics_v2(freqs, c1, c2, th1, th2, a["fc"], gl)
    g = m.get
    R.update(freqs=freqs, c1_db=c1, c2_db=c2, c1_n=n1, c2_n=n2, th1=th1, th2=th2, metrics=m)
    R["platform_ok"] = bool(g("c1_lo_platform_rmse", 99) < 0.5 and g("c2_lo_platform_rmse", 99) < 0.5
                            and g("c1_hi_platform_rmse", 99) < 0.5
                            and g("c2_hi_platform_rmse", 99) < 0.5)
    R["slope_ok"] = bool(g("c1_slope_rmse", 99) < 1.0 and g("c2_slope_rmse", 99) < 1.0)
    R["fc_ok"] = bool(g("c1_fc_error", 99) < 0.5 and g("c2_fc_error", 99) < 0.5)
    R["spectrum_pass"] = R["platform_ok"] and R["slope_ok"] and R["fc_ok"]
    ti = tilt_index(x2, y2, sr, codes, levels, a["n_fft"], a["hop"], a["level_percentile"], dtype)
    R["ti_data"], R["ti"] = ti, tilt_stats(ti)
    R["ti_effect"] = R["ti"].get("ti_effect", 0)
    R["ok"] = bool(R["eng_pass"] and R["spectrum_pass"] and R["c2_ratio_ok"])
    return R


def report_v2(R):
    w = lambda b: "PASS" if b else "FAIL"  # noqa: E731
    t = R["ti"].get
    L = ["Tomatis ±15dB 自适应验证报告 v2", "=" * 50, "\nA. 工程检查", f"  结果: {w(R['eng_pass'])}",
         f"  峰值: {R['peak']:.4f}", "\nB. 自适应门控", f"  最优阈值 T: {R['T']:.2f} dBFS",
         f"  C2 占比: {R['ratio']*100:.1f}%", f"  切换次数: {R['switch_count']}",
         "\nC. 条件频谱验证", f"  有效帧: C1={R['c1_n']}, C2={R['c2_n']}",
         f"  平台 RMSE: {w(R['platform_ok'])}", f"  斜坡 RMSE: {w(R['slope_ok'])}",
         f"  fc 误差: {w(R['fc_ok'])}", "\nD. 效果量化", f"  C1 TI: {t('c1_mean', 0):.2f} dB",
         f"  C2 TI: {t('c2_mean', 0):.2f} dB", f"  分离度: {R['ti_effect']:.2f} dB",
         "\n" + "=" * 50, f"总体结果: {w(R['ok'])}"]
    return "\n".join(L)


def csv_columns(R):
    """The four value columns as the CSV's '%.4f' text reads back."""
    cols = np.stack([R["c1_db"], R["th1"] if "th1" in R else R["c1_theory"],
                     R["c2_db"], R["th2"] if "th2" in R else R["c2_theory"]], axis=1)
    return np.array([[float(f"{v:.4f}") for v in row] for row in cols.tolist()])


def run_l1(x, y, sr, rows, a, frames_in=None, frames_out=None, dtype=np.float32):
    """validate_layer1 on arrays, the state-CSV rows (arrays) and the argument dict."""
    x2, y2 = _2d(x, np.float32), _2d(y, np.float32)
    n_in = len(x2) if frames_in is None else frames_in
    n_out = len(y2) if frames_out is None else frames_out
    R = {}
    R["peak"] = np.float32(np.max(np.abs(y2)))
    R["eng_pass"] = bool(x2.shape[1] == y2.shape[1] and n_in == n_out and R["peak"] < 0.98)
    T = a["gate_scale"] * a["gate_ui"] + a["gate_offset"]
    levels, starts = frame_levels(x2, a["n_fft"], a["hop"])
    sim = gate(levels, starts, T + a["hyst_db"] / 2, T - a["hyst_db"] / 2,
               int(a["up_delay_ms"] * sr / 1000))
    cs = np.asarray(rows["state"], np.int8)
    n = min(len(cs), len(sim))
    R.update(levels=levels, sim=sim, total=n, mismatch=int(np.count_nonzero(cs[:n] != sim[:n])),
             csv_switches=switches(cs), sim_switches=switches(sim))
    d = np.abs(np.asarray(rows["level_dbfs"], np.float64)[:n] - levels[:n])
    R["level_max_diff"] = float(d.max()) if n else 0
    R["mismatch_rate"] = R["mismatch"] / n if n else 0
    R["gate_ok"] = bool(R["mismatch_rate"] < 0.01 and R["level_max_diff"] < 0.1)
    freqs, c1, c2, n1, n2 = conditional_l1(x2, y2, sr, cs, a["n_fft"], a["hop"], -60, dtype)
    th1 = tilt_gain_db(freqs, a["fc"], a["slope"], a["c1_low"], a["c1_high"])
    th2 = tilt_gain_db(freqs, a["fc"], a["slope"], a["c2_low"], a["c2_high"])
    rm = []
    for meas, th in ((c1, th1), (c2, th2)):
        for lo, hi in ((100, 800), (800, 1200), (2000, 8000)):
            k = (freqs >= lo) & (freqs <= hi)
            rm.append(np.sqrt(np.mean((meas[k] - th[k]) ** 2)) if np.any(k) else 0.0)
    R.update(freqs=freqs, c1_db=c1, c2_db=c2, c1_n=n1, c2_n=n2, th1=th1, th2=th2, rmse=rm)
    R["spectrum_ok"] = bool(max(rm) < 1.5)
    R["ok"] = bool(R["eng_pass"] and R["gate_ok"] and R["spectrum_ok"])
    return R


def rule_bound(e32, scale=1.0):
    """The project's rule for a device value against float64: 8 * max(the float32
    numpy statement's own error, 2^-23), relative to ``scale``."""
    return 8 * max(float(e32), 2.0 ** -23) * scale
