#!/usr/bin/env python3
"""Time of the audio resampler (``tomatis_resample_poly``, tm_resample.hip) on
one MI355X: a device-resident 60-minute stereo stream at 44.1 kHz (160 / 147),
96 kHz (1 / 2) and 192 kHz (1 / 4) to 48 kHz, and ``cut_audio`` file to file
with the workflow's arguments (cut 16.8 s, keep 1800 s, to 48 kHz).  Prints one
JSON line per rate and one for the file.

Method as tools/bench_envelope_rational.py: HIP events on the library's stream,
3 warm-up calls, the median of ``--runs`` (>= 20) calls.  The bytes are the
samples read once and the output written once, 4 ch (n + n_out); the copy
bandwidth is ``tomatis_copy_probe`` in the same process.  The baseline is what
the path was before: ``scipy.signal.resample_poly(x, up, down, axis=0)`` on one
core, on ONE MINUTE of the same stream, scaled by 60 (``cpu.scaled`` says so).
``--minutes`` shrinks the stream where the memory does not hold it.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, runs, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def bench_rate(a, sr, ch=2):
    import numpy as np
    import torch
    from tomatis_audio_processor_amd import resample
    from tomatis_audio_processor_amd._lib import check, lib, ptr, stream_handle
    up, down = resample.ratio(sr, 48000)
    n = int(a.minutes * 60 * sr)
    n_out = resample.n_out(n, up, down)
    h, st = lib(), stream_handle()
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = (torch.rand((n, ch), generator=g, device="cuda", dtype=torch.float32) - 0.5)
    taps = torch.from_numpy(resample.taps(up, down).copy()).cuda()
    out = torch.empty((n_out, ch), dtype=torch.float32, device="cuda")

    flat = x.reshape(-1)
    cp_src = flat[: min(flat.numel() // 4, 1 << 27) * 4]
    cp_dst = torch.empty_like(cp_src)
    cp_ms, _, _ = timed(torch, lambda: check(h.tomatis_copy_probe(
        ptr(cp_src), ptr(cp_dst), cp_src.numel(), st), "copy_probe"), a.runs, a.warmup)
    copy_gbs = 2.0 * 4.0 * cp_src.numel() / (cp_ms * 1e-3) / 1e9
    del cp_dst

    def run():
        check(h.tomatis_resample_poly(ptr(x), n, 0, n, ch, up, down, ptr(taps), taps.numel(),
                                      ptr(out), st), "resample_poly")

    ms, lo, hi = timed(torch, run, a.runs, a.warmup)
    nbytes = 4 * ch * (n + n_out)
    gbs = nbytes / (ms * 1e-3) / 1e9
    cpu = None
    if not a.no_cpu:
        from scipy.signal import resample_poly
        piece = x[: 60 * sr].cpu().numpy()
        cores = None
        try:
            cores = os.sched_getaffinity(0)
            os.sched_setaffinity(0, {sorted(cores)[0]})  # one core
        except (AttributeError, OSError):
            pass
        t0 = time.perf_counter()
        y = resample_poly(piece, up, down, axis=0)
        one = time.perf_counter() - t0
        if cores:
            os.sched_setaffinity(0, cores)
        dev = out[: len(y) - 64].cpu().numpy()   # away from the piece's own end
        err = float(np.max(np.abs(dev - y[: len(dev)])))
        scaled_s = one * n / (60 * sr)
        cpu = dict(one_minute_s=round(one, 3), scaled_s=round(scaled_s, 2),
                   scaled=f"one minute measured, scaled by {n / (60 * sr):g}",
                   speedup=round(scaled_s * 1e3 / ms, 1), max_abs_diff_first_minute=err)
    print(json.dumps(dict(
        fn="resample_poly", workload=f"{a.minutes:g} min {ch}-channel {sr} Hz -> 48000 Hz",
        ratio=[up, down], frames=n, out_frames=n_out,
        outputs_per_workgroup=resample.outputs_per_workgroup(up, down, ch),
        ms=dict(median=round(ms, 4), min=round(lo, 4), max=round(hi, 4), runs=a.runs),
        bytes=nbytes, gbs=round(gbs, 1), achievable_peak_gbs=round(copy_gbs, 1),
        frac_of_copy=round(gbs / copy_gbs, 3),
        cpu_how="scipy.signal.resample_poly(axis=0), float32, one core", cpu=cpu)), flush=True)


def bench_file(a):
    import torch
    from tomatis_audio_processor_amd import cut_tomatis_d, fileio
    sr, ch = 44100, 2
    n = int((a.file_minutes * 60 + 16.8) * sr)
    g = torch.Generator(device="cuda").manual_seed(99)
    x = (torch.rand(n * ch, generator=g, device="cuda", dtype=torch.float32) - 0.5) * 0.5
    with tempfile.TemporaryDirectory() as d:
        inp, out = os.path.join(d, "in.flac"), os.path.join(d, "out.flac")
        fileio.write_device(inp, x, n, ch, sr, log=lambda *s: None)
        del x
        import contextlib
        import io
        ts = []
        for _ in range(a.file_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                frames, out_sr = cut_tomatis_d.cut_audio(inp, out, 16.8, a.file_minutes * 60, 48000)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print(json.dumps(dict(
            fn="cut_audio", workload=f"{a.file_minutes:g} min stereo 44100 Hz FLAC (white noise), "
            "cut 16.8 s, to 48000 Hz, file to file", out_frames=frames, out_sr=out_sr,
            in_bytes=os.path.getsize(inp), out_bytes=os.path.getsize(out),
            wall_s=dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3),
                        max=round(max(ts), 3), runs=a.file_runs))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rates", type=int, nargs="+", default=[44100, 96000, 192000])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_cpu", action="store_true")
    ap.add_argument("--file_minutes", type=float, default=30.0)
    ap.add_argument("--file_runs", type=int, default=3)
    ap.add_argument("--no_file", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs an MI355X: there is no CPU fallback")
    for sr in a.rates:
        bench_rate(a, sr)
        torch.cuda.empty_cache()
    if not a.no_file:
        bench_file(a)


if __name__ == "__main__":
    main()
