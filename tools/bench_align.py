#!/usr/bin/env python3
"""Time of the delay estimate on one MI355X:
``align.find_delay`` on a device-resident 60-minute 48 kHz stereo pair (the C2
length) with the reference's defaults (2 kHz envelopes, the middle 25 s of the
base), next to the host scipy body (``align._find_delay_host``, one core) on
the same pair.  Prints one JSON line.

Method: HIP events on the library's stream, warm-up, median of ``--runs``
(>= 20) calls; the same for every entry point on its own (called directly).
The envelope's bytes are the PCM read once plus the envelope written, read by
the sum, read and written by the centring; the copy bandwidth is
``tomatis_copy_probe`` in the same process (bench.py's
roofline.achievable_peak).  The correlation's work is (nt - nb + 1) * nb
fused multiply-adds, against the 157.3 TFLOP/s float32 vector peak of the
data sheet.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_PEAK_TFLOPS = 157.3


def make_pair(torch, n: int, shift: int, seed: int):
    """Noise under a random 50 Hz amplitude contour; the base starts ``shift``
    samples into the material the target plays from its start."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = n + shift
    amp = 0.02 + 0.3 * torch.rand((m // 960 + 2,), generator=g, device="cuda")
    amp = torch.repeat_interleave(amp, 960)[:m].reshape(m, 1)
    u = torch.randn((m, 2), generator=g, device="cuda", dtype=torch.float32)
    u.mul_(amp).clamp_(-1.0, 1.0)
    return u[:n].contiguous(), u[shift:shift + n].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--shift", type=int, default=123456)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_cpu", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import torch
    from tomatis_audio_processor_amd import align
    from tomatis_audio_processor_amd._lib import (ALIGN_MEAN_DOUBLES, check, lib, ptr,
                                                  stream_handle)
    if not torch.cuda.is_available():
        raise SystemExit("bench_align needs an MI355X: there is no CPU fallback")

    sr, ds_sr, chunk_sec = a.sr, 2000, 25.0
    n = int(a.minutes * 60 * sr)
    xt, xb = make_pair(torch, n, a.shift, 777)
    h, st = lib(), stream_handle()

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
    total = timed(lambda: align.find_delay(xt, xb, sr=sr, ds_sr=ds_sr, chunk_sec=chunk_sec))

    # every entry point on its own
    down = sr // ds_sr
    s, e = align._chunk(n, sr, chunk_sec)
    taps = torch.from_numpy(align._taps(down)).cuda()
    mean = torch.empty(ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
    nt, nb = -(-n // down), -(-(e - s) // down)
    mt = torch.empty(nt, dtype=torch.float32, device="cuda")
    mb = torch.empty(nb, dtype=torch.float32, device="cuda")
    corr = torch.empty(nt - nb + 1, dtype=torch.float32, device="cuda")
    idx = torch.empty(1, dtype=torch.int64, device="cuda")
    val = torch.empty(1, dtype=torch.float32, device="cuda")

    def env(x, start, ln, out):
        check(h.tomatis_align_envelope(ptr(x), n, start, ln, down, ptr(taps), taps.numel(),
                                       ptr(out), ptr(mean), st), "align_envelope")

    parts = {}

    def add(name, fn, nbytes=None, macs=None):
        ms, lo, hi = timed(fn)
        d = dict(ms=round(ms, 4), min=round(lo, 4), max=round(hi, 4))
        if nbytes is not None:
            d.update(bytes=nbytes, gbs=round(nbytes / (ms * 1e-3) / 1e9, 1),
                     frac_of_copy=round(nbytes / (ms * 1e-3) / 1e9 / copy_gbs, 3))
        if macs is not None:
            tf = 2.0 * macs / (ms * 1e-3) / 1e12
            d.update(macs=macs, tflops=round(tf, 2), frac_of_fp32_peak=round(tf / FP32_PEAK_TFLOPS, 3))
        parts[name] = d

    add("envelope target", lambda: env(xt, 0, n, mt), nbytes=8 * n + 4 * 4 * nt)
    add("envelope base chunk", lambda: env(xb, s, e - s, mb), nbytes=8 * (e - s) + 4 * 4 * nb)
    add("xcorr", lambda: check(h.tomatis_align_xcorr(ptr(mt), nt, ptr(mb), nb, ptr(corr), st),
                               "align_xcorr"), macs=(nt - nb + 1) * nb)
    add("argmax", lambda: check(h.tomatis_align_argmax(ptr(corr), corr.numel(), ptr(idx),
                                                       ptr(val), st), "align_argmax"),
        nbytes=4 * corr.numel())

    cpu_s, cpu_delay = None, None
    if not a.no_cpu:
        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # one core
        except (AttributeError, OSError):
            pass
        ht, hb = xt.cpu().numpy(), xb.cpu().numpy()
        t0 = time.perf_counter()
        cpu_delay = align._find_delay_host(ht, hb, sr, ds_sr, chunk_sec)
        cpu_s = time.perf_counter() - t0

    print(json.dumps(dict(
        fn="find_delay", workload=f"{a.minutes:g} min stereo {sr} Hz pair, shift {a.shift}",
        frames=n, envelope_samples=[nt, nb], delay=delay,
        find_delay_ms=dict(median=round(total[0], 3), min=round(total[1], 3),
                           max=round(total[2], 3), runs=a.runs),
        achievable_peak_gbs=round(copy_gbs, 1), fp32_peak_tflops=FP32_PEAK_TFLOPS,
        entry_points_ms_sum=round(sum(p["ms"] for p in parts.values()), 3),
        entry_points=parts,
        cpu_scipy_s=None if cpu_s is None else round(cpu_s, 3),
        cpu_how="align._find_delay_host (scipy resample_poly + fftconvolve), one core, same pair",
        cpu_delay=cpu_delay,
        speedup=None if cpu_s is None else round(cpu_s * 1e3 / total[0], 1))), flush=True)


if __name__ == "__main__":
    main()
