#!/usr/bin/env python3
"""Time of compare_audio on the device on one MI355X:
device-resident 30- and 60-minute 48 kHz stereo pairs, every new entry point
on its own (called directly), ``align.find_delay_full`` and ``compare_audio.
compare`` end to end, next to the reference's scipy body of the delay estimate
(``align._find_delay_full_host``: resample_poly + fftconvolve(full) + argmax,
one core) on the same pair in the same run.  Prints one JSON line.

Method: HIP events on the library's stream, warm-up, median of ``--runs``
(>= 20) calls.  The FFT's algorithmic bytes are its passes (5 of the six-step
scheme above 8192 points, 1 below) times L * 8 B read and written, set against
the copy bandwidth ``tomatis_copy_probe`` reaches in the same process.  The
direct correlation the FFT path replaces would be nc * nb fused multiply-adds;
at the rate tomatis_align_xcorr reaches that is the
``direct_at_97_tflops_s`` figure.

``--fft_only P``: nothing but ``--runs`` forward transforms of 2^P points, for a
kernel trace of the passes.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_align import make_pair  # noqa: E402

XCORR_DIRECT_TFLOPS = 97.0   # DESIGN.md §7d, tomatis_align_xcorr at nb = 50000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[30.0, 60.0])
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--shift", type=int, default=123456)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_cpu", action="store_true")
    ap.add_argument("--fft_only", type=int, default=0)
    a = ap.parse_args()
    if a.runs < 20 and not a.fft_only:
        ap.error("--runs must be at least 20")

    import ctypes as C
    import torch
    from tomatis_audio_processor_amd import align, compare_audio
    from tomatis_audio_processor_amd._lib import (ALIGN_MEAN_DOUBLES, RESIDUAL_DOUBLES, check, lib,
                                                  ptr, stream_handle)
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare needs an MI355X: there is no CPU fallback")
    h, st = lib(), stream_handle()

    def fft_buffers(p):
        x = torch.randn(2 << p, dtype=torch.float32, device="cuda")
        y = torch.empty_like(x)
        w = torch.empty(int(h.tomatis_fft_pow2_work_bytes(p)), dtype=torch.uint8, device="cuda")
        return x, y, w

    if a.fft_only:
        x, y, w = fft_buffers(a.fft_only)
        for _ in range(a.runs):
            check(h.tomatis_fft_pow2(ptr(x), ptr(y), a.fft_only, 0, ptr(w), st), "fft_pow2")
        torch.cuda.synchronize()
        return

    def timed(fn, runs=a.runs, warm=a.warmup):
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

    sr, ds_sr = a.sr, 2000
    down = sr // ds_sr
    results = []
    for minutes in a.minutes:
        n = int(minutes * 60 * sr)
        xc, xb = make_pair(torch, n, a.shift, 777)       # the candidate starts later

        flat = xc.reshape(-1)
        cp_src = flat[: min(flat.numel() // 4, 1 << 27) * 4]
        cp_dst = torch.empty_like(cp_src)
        cp_ms, _, _ = timed(lambda: check(h.tomatis_copy_probe(ptr(cp_src), ptr(cp_dst),
                                                               cp_src.numel(), st), "copy_probe"))
        copy_gbs = 2.0 * 4.0 * cp_src.numel() / (cp_ms * 1e-3) / 1e9
        del cp_dst

        delay = align.find_delay_full(xb, xc, sr=sr, ds_sr=ds_sr)
        total = timed(lambda: align.find_delay_full(xb, xc, sr=sr, ds_sr=ds_sr))

        taps = torch.from_numpy(align._taps(down)).cuda()
        mean = torch.empty(ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
        ne = -(-n // down)
        eb = torch.empty(ne, dtype=torch.float32, device="cuda")
        ec = torch.empty(ne, dtype=torch.float32, device="cuda")
        n_lags = 2 * ne - 1
        p = max(4, (n_lags - 1).bit_length())
        L = 1 << p
        corr = torch.empty(n_lags, dtype=torch.float32, device="cuda")
        work = torch.empty(int(h.tomatis_align_xcorr_full_work_bytes(ne, ne)), dtype=torch.uint8,
                           device="cuda")
        idx = torch.empty(1, dtype=torch.int64, device="cuda")
        val = torch.empty(1, dtype=torch.float32, device="cuda")
        res = torch.empty(RESIDUAL_DOUBLES, dtype=torch.float64, device="cuda")
        fx, fy, fw = fft_buffers(p)
        parts = {}

        def add(name, fn, nbytes=None):
            ms, lo, hi = timed(fn)
            d = dict(ms=round(ms, 4), min=round(lo, 4), max=round(hi, 4))
            if nbytes is not None:
                d.update(bytes=nbytes, gbs=round(nbytes / (ms * 1e-3) / 1e9, 1),
                         frac_of_copy=round(nbytes / (ms * 1e-3) / 1e9 / copy_gbs, 3))
            parts[name] = d

        def env(x, out):
            check(h.tomatis_align_envelope_mean_first(ptr(x), n, 0, n, down, ptr(taps),
                                                      taps.numel(), ptr(out), ptr(mean), st),
                  "align_envelope_mean_first")

        env(xc, ec)
        add("envelope_mean_first", lambda: env(xb, eb), nbytes=2 * 8 * n + 4 * ne)
        passes = 5 if p > 13 else 1
        for inv in (0, 1):
            add("fft_pow2 " + ("inverse" if inv else "forward"),
                lambda: check(h.tomatis_fft_pow2(ptr(fx), ptr(fy), p, inv, ptr(fw), st), "fft"),
                nbytes=passes * 2 * 8 * L)
        add("xcorr_full", lambda: check(h.tomatis_align_xcorr_full(
            ptr(ec), ne, ptr(eb), ne, ptr(corr), ptr(work), st), "xcorr_full"))
        add("argmax", lambda: check(h.tomatis_align_argmax(ptr(corr), n_lags, ptr(idx), ptr(val),
                                                           st), "argmax"), nbytes=4 * n_lags)
        m = n - abs(delay)
        b2, c2 = compare_audio.align_pair(xb, xc, delay)
        add("compare_residual", lambda: check(h.tomatis_compare_residual(
            ptr(b2), ptr(c2), m, C.c_float(1.0), ptr(res), st), "residual"), nbytes=2 * 8 * m)
        del fx, fy, fw, work

        quiet = lambda s: None  # noqa: E731
        out = compare_audio.compare(xb, xc, sr, log=quiet)
        t0 = time.perf_counter()
        compare_audio.compare(xb, xc, sr, log=quiet)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        cmp_ms = timed(lambda: compare_audio.compare(xb, xc, sr, log=quiet))

        cpu_s, cpu_delay = None, None
        if not a.no_cpu:
            try:
                os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # one core
            except (AttributeError, OSError):
                pass
            hb, hc = xb.cpu().numpy(), xc.cpu().numpy()
            t0 = time.perf_counter()
            cpu_delay = align._find_delay_full_host(hb, hc, sr, ds_sr)
            cpu_s = time.perf_counter() - t0
            del hb, hc
        direct_s = 2.0 * ne * ne / (XCORR_DIRECT_TFLOPS * 1e12)
        results.append(dict(
            workload=f"{minutes:g} min stereo {sr} Hz pair, shift {a.shift}", frames=n,
            envelope_samples=ne, fft_log2=p, fft_passes=passes, delay=delay,
            find_delay_full_ms=dict(median=round(total[0], 3), min=round(total[1], 3),
                                    max=round(total[2], 3), runs=a.runs),
            compare_ms=dict(median=round(cmp_ms[0], 3), min=round(cmp_ms[1], 3),
                            max=round(cmp_ms[2], 3), wall_s=round(wall, 4)),
            compare_result=dict(delay=out[2], gain_db=round(out[3], 4), snr_db=round(out[4], 3)),
            achievable_peak_gbs=round(copy_gbs, 1), entry_points=parts,
            direct_fmas=ne * ne, direct_at_97_tflops_s=round(direct_s, 4),
            xcorr_full_vs_direct=round(direct_s * 1e3 / parts["xcorr_full"]["ms"], 1),
            cpu_scipy_s=None if cpu_s is None else round(cpu_s, 3), cpu_delay=cpu_delay,
            speedup_find_delay=None if cpu_s is None else round(cpu_s * 1e3 / total[0], 1)))
        del xb, xc, b2, c2, eb, ec, corr
        torch.cuda.empty_cache()

    print(json.dumps(dict(
        fn="compare_audio", runs=a.runs, warmup=a.warmup,
        cpu_how="align._find_delay_full_host (scipy resample_poly + fftconvolve full + argmax), "
                "one core, same pair", results=results)), flush=True)


if __name__ == "__main__":
    main()
