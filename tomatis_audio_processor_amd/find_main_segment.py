"""Main-segment finder on the device — MI355X drop-in for src/find_main_segment.py
(workflow step 2.1): where in a recording the music
starts and ends, from windowed RMS levels against a p10 noise floor.

  reference (find_main_segment.py)                 here
  ------------------------------------------------ -----------------------------
  win_rms_dbfs :5-10 over the hop grid :57-72,      tomatis_an_frame_power_mean
  ``p`` and ``np.mean(p)``                          (all windows, one launch, bit-exact)
  ``+ EPS``, sqrt, ``+ EPS``, log10, ``20 *`` :9-10  host, the same numpy scalar calls
  np.percentile :84, ``>=`` :87, find_segments      host, the same numpy calls
  :12-26, the longest run and the pads :93-112

The device forms the F window means; numpy's float32 log10 is not correctly
rounded and stays with numpy, scalar by scalar as the reference calls it, so
the installed numpy's promotion rules apply to both alike.  ``find_main_segment``
returns everything ``main`` prints.  There is no CPU fallback.
"""
from __future__ import annotations

import argparse

import numpy as np

from ._lib import check, lib, ptr, stream_handle

EPS = 1e-12
MAX_WIN = 65536  # tm_analysis.hip kMaxMeanWin


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("find_main_segment needs a ROCm GPU (MI355X)")
    return torch


def _load(x_or_path, sr):
    """-> (flat float32 cuda tensor, n, ch, sr)."""
    torch = _torch()
    if isinstance(x_or_path, str):
        from . import fileio
        return fileio.read_device(x_or_path)
    if sr is None:
        raise ValueError("sr is required with an array or a tensor")
    x = x_or_path
    if isinstance(x, torch.Tensor):
        t = x.to(device="cuda", dtype=torch.float32)
    else:
        a = np.ascontiguousarray(x, dtype=np.float32)
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    n, ch = t.shape
    return t.contiguous().reshape(-1), n, ch, int(sr)


def frame_power_mean(x, n: int, win: int, hop: int):
    """``np.mean((l * l + r * r) * 0.5)`` of every window of the flat stereo cuda
    tensor x ([n * 2]): float32 cuda tensor of 1 + (n - win) // hop values."""
    torch = _torch()
    if win < 1 or hop < 1:
        raise ValueError("win and hop must be at least one sample")
    if win > MAX_WIN:
        raise ValueError(f"win={win}: the device takes windows of at most {MAX_WIN} samples")
    F = 1 + (n - win) // hop if n >= win else 0
    out = torch.empty(F, dtype=torch.float32, device="cuda")
    if F:
        check(lib().tomatis_an_frame_power_mean(ptr(x), n, win, hop, ptr(out), stream_handle()),
              "an_frame_power_mean")
    return out


def find_segments(active: np.ndarray):
    """Runs of True as (start, end_exclusive) pairs."""
    a = np.concatenate(([False], np.asarray(active, bool), [False]))
    d = np.flatnonzero(a[1:] != a[:-1])
    return [(int(i), int(j)) for i, j in zip(d[::2], d[1::2])]


def find_main_segment(x_or_path, sr=None, win_ms=100.0, hop_ms=50.0, margin_db=15.0,
                      min_seg_sec=60.0, pad_sec=0.5):
    """The reference's decisions as a dict: ``sr``, ``dur``, ``ch``, ``levels``
    (float32), ``noise_floor``, ``thr``, ``t0``, ``t1``, ``len``, ``t0p``,
    ``t1p`` and ``status`` ("ok", "none": no active window, "short": the longest
    run is under ``min_seg_sec``; the fields not reached are None)."""
    x, n_total, ch, sr = _load(x_or_path, sr)
    dur = n_total / sr
    if ch != 2:
        raise ValueError(f"期望双声道，实际 {ch}")
    win = int(sr * win_ms / 1000.0)
    hop = int(sr * hop_ms / 1000.0)
    win_sec = win / sr
    means = frame_power_mean(x, n_total, win, hop).cpu().numpy()
    levels = []
    times = []
    next_start = 0
    for m in means:  # m: np.float32, as np.mean(p) is
        r = np.sqrt(m + EPS)
        levels.append(float(20.0 * np.log10(r + EPS)))
        times.append(next_start / sr)
        next_start += hop
    levels = np.array(levels, np.float32)
    times = np.array(times, np.float32)

    res = dict(sr=sr, dur=dur, ch=ch, levels=levels, noise_floor=None, thr=None, t0=None, t1=None,
               len=None, t0p=None, t1p=None, status="none")
    noise_floor = float(np.percentile(levels, 10))
    thr = noise_floor + margin_db
    res.update(noise_floor=noise_floor, thr=thr)
    active = levels >= thr
    segs = find_segments(active)
    if not segs:
        return res
    best = None
    best_len = -1.0
    for i, j in segs:
        t0 = float(times[i])
        t1 = float(times[j - 1] + win_sec)
        L = t1 - t0
        if L > best_len:
            best_len = L
            best = (t0, t1)
    t0, t1 = best
    res.update(t0=t0, t1=t1, len=best_len, status="short")
    if best_len < min_seg_sec:
        return res
    res.update(t0p=max(0.0, t0 - pad_sec), t1p=min(dur, t1 + pad_sec), status="ok")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("--win_ms", type=float, default=100.0, help="窗口长度（ms）")
    ap.add_argument("--hop_ms", type=float, default=50.0, help="步长（ms）")
    ap.add_argument("--margin_db", type=float, default=15.0, help="高于噪声底多少dB算有音乐")
    ap.add_argument("--min_seg_sec", type=float, default=60.0, help="最短主段长度（秒）")
    ap.add_argument("--pad_sec", type=float, default=0.5, help="裁剪前后额外保留（秒）")
    args = ap.parse_args(argv)
    r = find_main_segment(args.input, None, args.win_ms, args.hop_ms, args.margin_db,
                          args.min_seg_sec, args.pad_sec)
    if r["status"] == "none":
        print("未找到主音乐段：请调低 margin_db 或检查音频是否几乎全静音。")
        return
    if r["status"] == "short":
        print(f"最长段只有 {r['len']:.1f}s，小于 min_seg_sec={args.min_seg_sec}，建议调参。")
        return
    print("==== 自动检测结果 ====")
    print(f"总时长: {r['dur']:.2f}s  采样率: {r['sr']}Hz  声道: {r['ch']}")
    print(f"噪声底(p10): {r['noise_floor']:.1f} dBFS")
    print(f"活动阈值: {r['thr']:.1f} dBFS (noise_floor + {args.margin_db}dB)")
    print(f"主音乐段(未加pad): start={r['t0']:.3f}s  end={r['t1']:.3f}s  len={r['len']:.1f}s")
    print(f"建议裁剪(加pad):  start={r['t0p']:.3f}s  end={r['t1p']:.3f}s  "
          f"len={(r['t1p'] - r['t0p']):.1f}s")


if __name__ == "__main__":
    main()
