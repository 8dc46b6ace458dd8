"""Cut the head off a recording, on the device — MI355X drop-in for
src/cut_tomatis_d.py (workflow step 2.1).

With ``duration_seconds`` and ``target_sr`` left at None this is the reference:
the same prints, ``cut_samples = int(cut_seconds * sr)``, FLAC PCM_24 out, the
same three ``sys.argv`` forms.  The two extra arguments (a fourth and fifth
positional on the command line) make it the workflow's
``ffmpeg -ss 16.80 -t 1800 -ar 48000``: keep ``int(duration_seconds * sr)``
frames after the cut (fewer at the end of the file) and resample the kept range
to ``target_sr`` with ``resample.resample_to``, whose start / stop are that
range, so nothing is copied.  Each prints one extra line when given.

The file stays on the device: ``fileio.read_device`` decodes, ``write_device``
quantises with libsndfile's rule (resampler overshoot above full scale clips as
libsndfile would) and encodes.  There is no CPU fallback.
"""
from __future__ import annotations

import sys

from . import fileio, resample


def cut_audio(input_path, output_path, cut_seconds=16.0, duration_seconds=None, target_sr=None):
    """Drop the first ``cut_seconds`` of ``input_path`` and write FLAC PCM_24 to
    ``output_path``; optionally keep ``duration_seconds`` and resample to
    ``target_sr``.  Returns (frames written, sample rate written)."""
    print(f"正在读取: {input_path}")

    x, n, ch, sr = fileio.read_device(input_path)

    print(f"采样率: {sr} Hz")
    print(f"声道数: {ch}")
    print(f"原始长度: {n} 采样点 ({n/sr:.2f} 秒)")

    cut_samples = int(cut_seconds * sr)
    start = min(cut_samples, n) if cut_samples >= 0 else max(0, n + cut_samples)  # x[cut:]
    stop = n
    if duration_seconds is not None:
        stop = min(n, start + max(0, int(duration_seconds * sr)))
    n_cut = stop - start

    print(f"\n裁剪 {cut_seconds} 秒 ({cut_samples} 采样点)")
    if duration_seconds is not None:
        print(f"保留 {duration_seconds} 秒 ({n_cut} 采样点)")
    print(f"裁剪后长度: {n_cut} 采样点 ({n_cut/sr:.2f} 秒)")

    out_sr = sr
    if target_sr is not None and int(target_sr) != sr and n_cut > 0:
        y = resample.resample_to(x.reshape(n, ch), sr, int(target_sr), start, stop)
        out_sr, n_cut = int(target_sr), y.shape[0]
        y = y.reshape(-1)
    else:
        if target_sr is not None:
            out_sr = int(target_sr)
        y = x[start * ch:stop * ch]
    if target_sr is not None:
        print(f"重采样 {sr} Hz -> {out_sr} Hz: {n_cut} 采样点 ({n_cut/out_sr:.2f} 秒)")

    print(f"\n正在保存: {output_path}")
    fileio.write_device(output_path, y, n_cut, ch, out_sr, log=lambda *a, **k: None)

    print("✓ 完成")
    return n_cut, out_sr


def main(argv=None):
    argv = sys.argv if argv is None else argv
    duration_seconds = target_sr = None
    if len(argv) < 2:
        input_path = "Tomatis_D.flac"
        output_path = "Tomatis_D_cut16s.flac"
        cut_seconds = 16.0
    elif len(argv) == 2:
        input_path = argv[1]
        output_path = input_path.replace(".flac", "_cut16s.flac")
        cut_seconds = 16.0
    else:
        input_path = argv[1]
        output_path = argv[2]
        cut_seconds = float(argv[3]) if len(argv) > 3 else 16.0
        duration_seconds = float(argv[4]) if len(argv) > 4 else None
        target_sr = int(argv[5]) if len(argv) > 5 else None
    cut_audio(input_path, output_path, cut_seconds, duration_seconds, target_sr)


if __name__ == "__main__":
    main()
