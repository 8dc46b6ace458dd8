"""De-click stage on the device — MI355X drop-in for src/declick_inpaint.py
(``mad_sigma`` :7-11, ``merge_runs`` :13-24, ``inpaint_linear`` :26-46, CLI
:48-110): a MAD click detector over the sample-to-sample differences and linear
inpainting of the short segments it finds.

The whole step runs in ``csrc/tm_declick.hip`` and is bit-exact: the device
returns the two middle order statistics of each median as bit patterns, and
only the file's scalars (the even-count mean, ``+ 1e-12``, ``/ 0.6745``,
``k * sigma``) are formed here, with the numpy float32 scalar expressions the
reference evaluates.  ``declick`` is the function the CLI and other callers
share.  There is no CPU fallback.

Deviations from the reference, on purpose:

* negative ``pad_ms`` / ``merge_gap_ms`` raise ``ValueError`` before the GPU is
  touched (the reference's segments then overlap and its in-place loop depends
  on their order);
* fewer than two frames pass through unchanged (the reference does the same:
  its median of nothing is NaN and nothing hits);
* finite input is assumed, as decoded PCM always is.
"""
from __future__ import annotations

import argparse
from collections import namedtuple

import numpy as np

from ._lib import check, lib, ptr, stream_handle

EPS = 1e-12

DeclickResult = namedtuple("DeclickResult", "y segs raw hits sigma thr")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the de-click stage needs a ROCm GPU (MI355X)")
    return torch


def _device_2d(x):
    """x (numpy array or tensor, [N] or [N, C]) as a contiguous float32 cuda tensor [N, C]."""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) \
        else x
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[1] > 128:
        raise ValueError(f"expected samples [N, C] with 1 <= C <= 128, got {tuple(t.shape)}")
    return t.to(device="cuda", dtype=torch.float32).contiguous()


def _work(n_frames: int):
    torch = _torch()
    words = int(lib().tomatis_declick_work_words(n_frames))
    return torch.empty(words, dtype=torch.int32, device="cuda")


def _median(d, n: int, work, centered: bool, center) -> np.float32:
    """np.median of the n device floats d (of |d - center| when centered):
    exact selection on the device, numpy's even-count mean here."""
    torch = _torch()
    out = torch.empty(2, dtype=torch.int32, device="cuda")
    check(lib().tomatis_declick_select(ptr(d), n, int(centered), float(center), (n - 1) // 2,
                                       n // 2, ptr(work), ptr(out), stream_handle()),
          "declick_select")
    lo, hi = out.cpu().numpy().view(np.float32)
    if n % 2:
        return lo
    return np.float32(lo + hi) / np.float32(2)


def _sigma_of_nothing() -> float:
    """mad_sigma of no values at all (a file of fewer than two frames): NaN,
    by the reference's own numpy expressions so that even its bits agree."""
    import warnings
    none = np.zeros(0, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        med = np.median(none)
        mad = np.median(np.abs(none - med)) + EPS
    return float(mad / 0.6745)


def _mad_sigma_device(d, n: int, work) -> float:
    med = _median(d, n, work, False, 0.0)
    mad = _median(d, n, work, True, med) + EPS
    return float(mad / 0.6745)


def mad_sigma(x) -> float:
    """Robust scale of non-negative finite values: MAD -> sigma."""
    torch = _torch()
    t = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray)
         else x).to(device="cuda", dtype=torch.float32).reshape(-1).contiguous()
    n = t.numel()
    if n == 0:
        return _sigma_of_nothing()
    if bool((t < 0).any()):
        raise ValueError("mad_sigma on the device takes non-negative values (a detection statistic)")
    return _mad_sigma_device(t, n, _work(n))


def merge_runs(mask: np.ndarray, gap: int = 0) -> np.ndarray:
    """Runs of True in a host mask as [start, end) rows; runs whose distance is
    at most ``gap`` False samples merge."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    brk = np.flatnonzero(np.diff(idx) > gap + 1)
    first = np.concatenate(([0], brk + 1))
    last = np.concatenate((brk, [idx.size - 1]))
    return np.stack([idx[first], idx[last] + 1], axis=1).astype(np.int64)


def _inpaint(xd, yd, n: int, ch: int, segs_dev, n_segs: int):
    check(lib().tomatis_declick_inpaint(ptr(xd), ptr(yd), n, ch, ptr(segs_dev), n_segs,
                                        stream_handle()), "declick_inpaint")


def inpaint_linear(x, segs):
    """Linear interpolation over each segment [s, e) of x [N, C], on the
    device; the segments are disjoint and at least one sample apart (what the
    detector produces), so every end point is an original sample."""
    torch = _torch()
    xd = _device_2d(x)
    n, ch = xd.shape
    yd = xd.clone()
    s = np.ascontiguousarray(np.asarray(segs, dtype=np.int64).reshape(-1, 2))
    if len(s) and n:
        _inpaint(xd, yd, n, ch, torch.from_numpy(s).cuda(), len(s))
    return yd


def declick(x, sr, k=12.0, pad_ms=1.5, merge_gap_ms=0.5, max_fix_ms=8.0) -> DeclickResult:
    """Detect and inpaint clicks in x ([N, C] device tensor or numpy array).

    Returns ``(y, segs, raw, hits, sigma, thr)``: the repaired samples
    (device-resident, [N, C]), the kept segments (int64 [kept, 2] rows of
    [start, end)), the number of segments before the length filter, the number
    of hits, and the detector's scale and threshold."""
    if pad_ms < 0:
        raise ValueError(f"pad_ms must be >= 0, got {pad_ms}")
    if merge_gap_ms < 0:
        raise ValueError(f"merge_gap_ms must be >= 0, got {merge_gap_ms}")
    torch = _torch()
    xd = _device_2d(x)
    n, ch = xd.shape
    yd = xd.clone()
    none = np.zeros((0, 2), dtype=np.int64)
    if n < 2:
        sigma = _sigma_of_nothing()
        return DeclickResult(yd, none, 0, 0, sigma, k * sigma)
    pad = int(round(pad_ms * sr / 1000.0))
    gap = int(round(merge_gap_ms * sr / 1000.0))
    max_fix = int(round(max_fix_ms * sr / 1000.0))
    h, st = lib(), stream_handle()
    work = _work(n)
    d = torch.empty(n - 1, dtype=torch.float32, device="cuda")
    check(h.tomatis_declick_dmax(ptr(xd), n, ch, ptr(d), st), "declick_dmax")
    sigma = _mad_sigma_device(d, n - 1, work)
    thr = k * sigma
    # hit = dmax > thr compares in float32 (a Python float against a float32 array)
    thr_bits = int(np.float32(thr).view(np.uint32))
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    check(h.tomatis_declick_hits(ptr(d), n - 1, thr_bits, pad, gap, ptr(work), ptr(counts), st),
          "declick_hits")
    hits, raw = (int(v) for v in counts.cpu()[:2])
    if hits == 0:
        return DeclickResult(yd, none, 0, 0, sigma, thr)
    bounds = torch.empty(2 * raw, dtype=torch.int64, device="cuda")
    segs = torch.empty((raw, 2), dtype=torch.int64, device="cuda")
    check(h.tomatis_declick_segments(ptr(d), n - 1, thr_bits, pad, gap, max_fix, ptr(work), raw,
                                     ptr(bounds), ptr(segs), ptr(counts), st), "declick_segments")
    c = counts.cpu()
    if int(c[3]):
        raise RuntimeError(f"declick_segments: device error word {int(c[3])}")
    kept = int(c[2])
    _inpaint(xd, yd, n, ch, segs, kept)
    return DeclickResult(yd, segs[:kept].cpu().numpy(), raw, hits, sigma, thr)


def build_parser() -> argparse.ArgumentParser:
    """The reference CLI's flags, defaults and help strings (:49-56)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--k", type=float, default=12.0, help="阈值系数：越大越保守（建议 10-18）")
    ap.add_argument("--pad_ms", type=float, default=1.5, help="每个爆点左右扩展窗口（ms）")
    ap.add_argument("--merge_gap_ms", type=float, default=0.5, help="把相近爆点合并（ms）")
    ap.add_argument("--max_fix_ms", type=float, default=8.0,
                    help="单次修复最大长度（ms），更长就跳过以免误伤")
    ap.add_argument("--report_csv", default=None, help="可选：输出爆点区间列表 CSV")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.pad_ms < 0:
        raise ValueError(f"--pad_ms must be >= 0, got {args.pad_ms}")
    if args.merge_gap_ms < 0:
        raise ValueError(f"--merge_gap_ms must be >= 0, got {args.merge_gap_ms}")

    from . import fileio
    x, n, ch, sr = fileio.read_device(args.input)
    print(f"[LOAD] sr={sr}, shape={(n, ch)}")

    res = declick(x[:n * ch].reshape(n, ch), sr, k=args.k, pad_ms=args.pad_ms,
                  merge_gap_ms=args.merge_gap_ms, max_fix_ms=args.max_fix_ms)
    print(f"[DETECT] MAD-sigma={res.sigma:.6g}, thr={res.thr:.6g}, hits={res.hits}")

    quiet = lambda m: None  # noqa: E731
    if res.hits == 0:
        print("[DONE] 未检测到明显爆点，直接拷贝输出。")
        fileio.write_device(args.output, res.y.reshape(-1), n, ch, sr, log=quiet)
        return

    print(f"[SEGS] raw={res.raw}, kept={len(res.segs)} (drop long={res.raw - len(res.segs)})")

    if args.report_csv:
        import csv
        with open(args.report_csv, "w", newline="", encoding="utf-8") as f:
            w = csv.writer(f)
            w.writerow(["start_sample", "end_sample", "start_sec", "end_sec", "len_samples"])
            for s, e in res.segs:
                w.writerow([int(s), int(e), s / sr, e / sr, int(e - s)])
        print(f"[REPORT] wrote {args.report_csv}")

    written, _ = fileio.write_device(args.output, res.y.reshape(-1), n, ch, sr, log=quiet)
    print(f"[SAVE] {written}")


if __name__ == "__main__":
    main()


__all__ = ["declick", "DeclickResult", "mad_sigma", "merge_runs", "inpaint_linear", "build_parser",
           "main", "EPS"]
