#!/usr/bin/env python3
"""Time of the rational-ratio decimator (``tomatis_align_envelope_rational``,
tm_align.hip) and of the two delay estimates built on it, on one MI355X: a
device-resident 60-minute stereo pair at 44.1 kHz (20 / 441) and one at 192 kHz
(1 / 96), with the reference's defaults (2 kHz envelopes, the middle 25 s of the
base), next to the host scipy bodies (``align._find_delay_host``,
``align._find_delay_full_host``, one core) on the same pair.  Prints one JSON
line per rate.

Method as tools/bench_align.py: HIP events on the library's stream, 3 warm-up
calls, the median of ``--runs`` (>= 20) calls.  The envelope's bytes are the
PCM read once plus the envelope written, read by the sum, read and written by
the centring (mean-last), or the PCM read twice, by the sum and by the
decimator, plus the envelope written (mean-first); the copy bandwidth is
``tomatis_copy_probe`` in the same process (bench.py's
roofline.achievable_peak).  ``--minutes`` shrinks the pair where the memory
does not hold 60 minutes at 192 kHz (11 GB for the pair).
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


def bench_rate(a, sr):
    import torch
    from tomatis_audio_processor_amd import align
    from tomatis_audio_processor_amd._lib import (ALIGN_MEAN_DOUBLES, check, lib, ptr,
                                                  stream_handle)
    ds_sr, chunk_sec = 2000, 25.0
    free, _ = torch.cuda.mem_get_info()
    minutes = a.minutes
    while minutes > 1 and 4.5 * 8 * minutes * 60 * sr > free:  # the pair, the probe's copy, slack
        minutes /= 2
    n = int(minutes * 60 * sr)
    shift = int(a.shift_sec * sr) + 7
    xt, xb = make_pair(torch, n, shift, 777)
    h, st = lib(), stream_handle()
    up, down = align._ratio(sr, ds_sr)

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

    flat = xt.reshape(-1)
    cp_src = flat[: min(flat.numel() // 4, 1 << 27) * 4]
    cp_dst = torch.empty_like(cp_src)
    cp_ms, _, _ = timed(lambda: check(h.tomatis_copy_probe(ptr(cp_src), ptr(cp_dst),
                                                           cp_src.numel(), st), "copy_probe"))
    copy_gbs = 2.0 * 4.0 * cp_src.numel() / (cp_ms * 1e-3) / 1e9
    del cp_dst

    delay = align.find_delay(xt, xb, sr=sr, ds_sr=ds_sr, chunk_sec=chunk_sec)
    t_valid = timed(lambda: align.find_delay(xt, xb, sr=sr, ds_sr=ds_sr, chunk_sec=chunk_sec))
    delay_full = align.find_delay_full(xb, xt, sr=sr, ds_sr=ds_sr)
    t_full = timed(lambda: align.find_delay_full(xb, xt, sr=sr, ds_sr=ds_sr))

    taps = torch.from_numpy(align._taps_rational(up, down)).cuda()
    mean = torch.empty(ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
    n_out = align._n_ds(n, up, down)
    out = torch.empty(n_out, dtype=torch.float32, device="cuda")
    mono = torch.sqrt(0.5 * (xt * xt).sum(dim=1) + 1e-12).contiguous()

    def env(x, channels, mean_first):
        check(h.tomatis_align_envelope_rational(ptr(x), n, 0, n, channels, up, down, ptr(taps),
                                                taps.numel(), mean_first, ptr(out), ptr(mean), st),
              "align_envelope_rational")

    parts = {}

    def add(name, fn, nbytes):
        ms, lo, hi = timed(fn)
        gbs = nbytes / (ms * 1e-3) / 1e9
        parts[name] = dict(ms=round(ms, 4), min=round(lo, 4), max=round(hi, 4), bytes=nbytes,
                           gbs=round(gbs, 1), frac_of_copy=round(gbs / copy_gbs, 3))

    add("stereo mean-last", lambda: env(xt, 2, 0), 8 * n + 4 * 4 * n_out)
    add("stereo mean-first", lambda: env(xt, 2, 1), 2 * 8 * n + 4 * n_out)
    add("1-D mean-last", lambda: env(mono, 1, 0), 4 * n + 4 * 4 * n_out)
    add("1-D mean-first", lambda: env(mono, 1, 1), 2 * 4 * n + 4 * n_out)
    del mono

    cpu = {}
    if not a.no_cpu:
        ht, hb = xt.cpu().numpy(), xb.cpu().numpy()
        cores = None
        try:
            cores = os.sched_getaffinity(0)
            os.sched_setaffinity(0, {sorted(cores)[0]})  # one core
        except (AttributeError, OSError):
            pass
        t0 = time.perf_counter()
        cpu["find_delay"] = align._find_delay_host(ht, hb, sr, ds_sr, chunk_sec)
        cpu["find_delay_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        cpu["find_delay_full"] = align._find_delay_full_host(hb, ht, sr, ds_sr)
        cpu["find_delay_full_s"] = round(time.perf_counter() - t0, 3)
        if cores:
            os.sched_setaffinity(0, cores)
        del ht, hb
        cpu["speedup_find_delay"] = round(cpu["find_delay_s"] * 1e3 / t_valid[0], 1)
        cpu["speedup_find_delay_full"] = round(cpu["find_delay_full_s"] * 1e3 / t_full[0], 1)

    def med(t):
        return dict(median=round(t[0], 3), min=round(t[1], 3), max=round(t[2], 3), runs=a.runs)

    print(json.dumps(dict(
        fn="envelope_rational", workload=f"{minutes:g} min stereo {sr} Hz pair, shift {shift}",
        ratio=[up, down], frames=n, envelope_samples=n_out, delay=delay, delay_full=delay_full,
        find_delay_ms=med(t_valid), find_delay_full_ms=med(t_full),
        achievable_peak_gbs=round(copy_gbs, 1), entry_point=parts,
        cpu_how="align._find_delay_host / _find_delay_full_host (scipy resample_poly + "
                "fftconvolve), one core, same pair", cpu=cpu or None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rates", type=int, nargs="+", default=[44100, 192000])
    ap.add_argument("--shift_sec", type=float, default=2.5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_cpu", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_envelope_rational needs an MI355X: there is no CPU fallback")
    for sr in a.rates:
        bench_rate(a, sr)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
