"""Plain numpy statement of the main-segment finder (src/find_main_segment.py)
and of the cut (src/cut_tomatis_d.py) on arrays, the inputs of their golden
cases (tests/golden/segment_cases.py), and the fixture loader."""
from __future__ import annotations

import functools
import hashlib
import os

import numpy as np

from tests.golden.segment_cases import AMP, BY_NAME, QUIET
from tests.golden_util import GOLDEN_DIR

EPS = 1e-12


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def build_input(name):
    """float32 [n, ch] (mono cases too); shared between tests: do not write to it."""
    c = BY_NAME[name]
    n = int(round(c["dur"] * c["sr"]))
    rng = np.random.default_rng(c["seed"])
    env = np.full(n, QUIET)
    for a, b in c["loud"]:
        env[int(round(a * c["sr"])):int(round(b * c["sr"]))] = AMP
    x = rng.uniform(-1.0, 1.0, (n, c["ch"])) * env[:, None]
    x = (np.rint(x * 2.0 ** 23) / 2.0 ** 23).astype(np.float32)   # |k| < 2^22: a lossless PCM_24
    x.setflags(write=False)
    return x


def pcm24(x):
    """The integers libsndfile writes for float32 samples as PCM_24."""
    return np.clip(np.rint(np.asarray(x, np.float64) * (2 ** 23 - 1)), -2 ** 23,
                   2 ** 23 - 1).astype(np.int32)


def levels(x, sr, win_ms=100.0, hop_ms=50.0):
    """(levels float32, times float32, win_sec) of :5-10 and :44-82: every window
    that fits, the scalar expressions of win_rms_dbfs."""
    win = int(sr * win_ms / 1000.0)
    hop = int(sr * hop_ms / 1000.0)
    lv, tm = [], []
    s = 0
    while s + win <= len(x):
        f = x[s:s + win]
        p = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) * 0.5
        r = np.sqrt(np.mean(p) + EPS)
        lv.append(float(20.0 * np.log10(r + EPS)))
        tm.append(s / sr)
        s += hop
    return np.array(lv, np.float32), np.array(tm, np.float32), win / sr


def runs(active):
    out, i, n = [], 0, len(active)
    while i < n:
        if not active[i]:
            i += 1
            continue
        j = i
        while j < n and active[j]:
            j += 1
        out.append((i, j))
        i = j
    return out


def statement(x, sr, win_ms=100.0, hop_ms=50.0, margin_db=15.0, min_seg_sec=60.0, pad_sec=0.5):
    """-> dict(levels, noise_floor, thr, stdout): what the script computes and prints."""
    n, ch = x.shape
    dur = n / sr
    if ch != 2:
        raise ValueError(f"期望双声道，实际 {ch}")
    lv, tm, win_sec = levels(x, sr, win_ms, hop_ms)
    noise_floor = float(np.percentile(lv, 10))
    thr = noise_floor + margin_db
    res = dict(levels=lv, noise_floor=noise_floor, thr=thr)
    segs = runs(lv >= thr)
    if not segs:
        res["stdout"] = "未找到主音乐段：请调低 margin_db 或检查音频是否几乎全静音。\n"
        return res
    best, best_len = None, -1.0
    for i, j in segs:
        t0 = float(tm[i])
        t1 = float(tm[j - 1] + win_sec)
        if t1 - t0 > best_len:
            best_len, best = t1 - t0, (t0, t1)
    t0, t1 = best
    if best_len < min_seg_sec:
        res["stdout"] = f"最长段只有 {best_len:.1f}s，小于 min_seg_sec={min_seg_sec}，建议调参。\n"
        return res
    t0p = max(0.0, t0 - pad_sec)
    t1p = min(dur, t1 + pad_sec)
    res.update(t0=t0, t1=t1, t0p=t0p, t1p=t1p)
    res["stdout"] = "".join(line + "\n" for line in [
        "==== 自动检测结果 ====",
        f"总时长: {dur:.2f}s  采样率: {sr}Hz  声道: {ch}",
        f"噪声底(p10): {noise_floor:.1f} dBFS",
        f"活动阈值: {thr:.1f} dBFS (noise_floor + {margin_db}dB)",
        f"主音乐段(未加pad): start={t0:.3f}s  end={t1:.3f}s  len={best_len:.1f}s",
        f"建议裁剪(加pad):  start={t0p:.3f}s  end={t1p:.3f}s  len={(t1p - t0p):.1f}s"])
    return res


def cut_statement(x, sr, cut_seconds=16.0):
    """-> (the array written, the stdout with {in} / {out} for the paths)."""
    n, ch = x.shape
    cut = int(cut_seconds * sr)
    y = x[cut:]
    text = "".join(line + "\n" for line in [
        "正在读取: {in}", f"采样率: {sr} Hz", f"声道数: {ch}",
        f"原始长度: {n} 采样点 ({n / sr:.2f} 秒)",
        f"\n裁剪 {cut_seconds} 秒 ({cut} 采样点)",
        f"裁剪后长度: {len(y)} 采样点 ({len(y) / sr:.2f} 秒)",
        "\n正在保存: {out}", "✓ 完成"])
    return y, text


def cli_args(params):
    out = []
    for k, v in params.items():
        out += [f"--{k}", str(v)]
    return out
