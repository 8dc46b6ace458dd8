#!/usr/bin/env python3
"""Time of the de-click stage on one MI355X: ``declick()``
on a device-resident 30-minute 48 kHz stereo stream with ~200 seeded clicks,
next to the numpy statement of the same stage (tests/declick_ref.py, one core)
on the same input.  Prints one JSON line.

Method: HIP events on the library's stream, warm-up, median of ``--runs`` (>= 20)
calls; the same for every pass on its own (the library entry points called
directly), so a pass far from the copy bandwidth can be named.  The bytes are
the ones the pass structure moves, computed here from the
shapes; the copy bandwidth is ``tomatis_copy_probe`` on the same input in the
same process (bench.py's roofline.achievable_peak).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pass_bytes(n_frames: int, ch: int, hits: bool = True) -> dict:
    """Algorithmic HBM bytes of each pass (4-byte samples, dmax resident)."""
    n, d = n_frames, n_frames - 1
    b = {
        "copy y = x": 8 * ch * n,                 # read x, write y
        "dmax": 4 * ch * n + 4 * d,               # read x, write dmax
        "select median": 3 * 4 * d,               # three digit passes over dmax
        "select mad": 3 * 4 * d,                  # three digit passes, keys on the fly
        "hits (tile hits + head count)": 2 * 4 * d,
        "segments (bounds write)": 4 * d if hits else 0,
    }
    b["total"] = sum(b.values())
    return b


def make_input(torch, n: int, ch: int, sr: int, n_clicks: int, seed: int):
    """Sine + noise + seeded clicks, quantised to 24 bit, built on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / sr
    x = (0.2 * torch.sin(2 * np.pi * 440.0 * t)).to(torch.float32).reshape(n, 1).repeat(1, ch)
    del t
    x += 0.01 * torch.randn((n, ch), generator=g, device="cuda", dtype=torch.float32)
    pos = torch.randint(0, n, (n_clicks,), generator=g, device="cuda")
    amp = 0.3 + 0.3 * torch.rand((n_clicks,), generator=g, device="cuda")
    x[pos] += amp.reshape(-1, 1)
    q = torch.clamp(torch.round(x.double() * 8388608.0), -8388607, 8388607)
    return (q / 8388608.0).to(torch.float32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--ch", type=int, default=2)
    ap.add_argument("--clicks", type=int, default=200)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_cpu", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import torch
    from tomatis_audio_processor_amd import declick_inpaint as dc
    from tomatis_audio_processor_amd._lib import check, lib, ptr, stream_handle
    from tests import declick_ref as ref
    if not torch.cuda.is_available():
        raise SystemExit("bench_declick needs an MI355X: there is no CPU fallback")

    n, ch, sr = int(a.minutes * 60 * a.sr), a.ch, a.sr
    x = make_input(torch, n, ch, sr, a.clicks, 4242)
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

    # copy bandwidth of this process on this input (bench.py's probe)
    flat = x.reshape(-1)
    cp_src = flat[: min(flat.numel() // 4, 1 << 27) * 4]
    cp_dst = torch.empty_like(cp_src)
    cp_ms, _, _ = timed(lambda: check(h.tomatis_copy_probe(ptr(cp_src), ptr(cp_dst),
                                                           cp_src.numel(), st), "copy_probe"))
    copy_gbs = 2.0 * 4.0 * cp_src.numel() / (cp_ms * 1e-3) / 1e9
    del cp_dst

    # the whole stage, as callers run it (includes its four small host read-backs)
    res = dc.declick(x, sr)
    total_ms, total_min, total_max = timed(lambda: dc.declick(x, sr))
    bytes_ = pass_bytes(n, ch, hits=res.hits > 0)

    # every pass on its own
    work = dc._work(n)
    d = torch.empty(n - 1, dtype=torch.float32, device="cuda")
    out = torch.empty(2, dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    thr_bits = int(np.float32(res.thr).view(np.uint32))
    pad, gap, max_fix = (int(round(v * sr / 1000.0)) for v in (1.5, 0.5, 8.0))
    lo, hi = (n - 2) // 2, (n - 1) // 2
    check(h.tomatis_declick_dmax(ptr(x), n, ch, ptr(d), st), "dmax")
    med = float(dc._median(d, n - 1, work, False, 0.0))
    bounds = torch.empty(2 * max(res.raw, 1), dtype=torch.int64, device="cuda")
    segs = torch.empty((max(res.raw, 1), 2), dtype=torch.int64, device="cuda")
    passes = {
        "copy y = x": lambda: x.clone(),
        "dmax": lambda: check(h.tomatis_declick_dmax(ptr(x), n, ch, ptr(d), st), "dmax"),
        "select median": lambda: check(h.tomatis_declick_select(
            ptr(d), n - 1, 0, 0.0, lo, hi, ptr(work), ptr(out), st), "select"),
        "select mad": lambda: check(h.tomatis_declick_select(
            ptr(d), n - 1, 1, med, lo, hi, ptr(work), ptr(out), st), "select"),
        "hits (tile hits + head count)": lambda: check(h.tomatis_declick_hits(
            ptr(d), n - 1, thr_bits, pad, gap, ptr(work), ptr(counts), st), "hits"),
    }
    per_pass = {}
    for name, fn in passes.items():
        ms, _, _ = timed(fn)
        per_pass[name] = dict(ms=round(ms, 4), bytes=bytes_[name],
                              gbs=round(bytes_[name] / (ms * 1e-3) / 1e9, 1),
                              frac_of_copy=round(bytes_[name] / (ms * 1e-3) / 1e9 / copy_gbs, 3))
    if res.raw:
        name = "segments (bounds write)"
        ms, _, _ = timed(lambda: check(h.tomatis_declick_segments(
            ptr(d), n - 1, thr_bits, pad, gap, max_fix, ptr(work), res.raw, ptr(bounds),
            ptr(segs), ptr(counts), st), "segments"))
        per_pass[name] = dict(ms=round(ms, 4), bytes=bytes_[name],
                              gbs=round(bytes_[name] / (ms * 1e-3) / 1e9, 1),
                              frac_of_copy=round(bytes_[name] / (ms * 1e-3) / 1e9 / copy_gbs, 3))
    kernel_ms = sum(p["ms"] for p in per_pass.values())

    cpu_s, same = None, None
    if not a.no_cpu:
        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # one core
        except (AttributeError, OSError):
            pass
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        want = ref.declick(xh, sr)
        cpu_s = time.perf_counter() - t0
        same = bool(np.array_equal(want["y"].view(np.uint32),
                                   res.y.cpu().numpy().view(np.uint32))
                    and np.array_equal(want["segs"], res.segs)
                    and (want["hits"], want["raw"]) == (res.hits, res.raw)
                    and ref.f64_bits(want["sigma"]) == ref.f64_bits(res.sigma))

    print(json.dumps(dict(
        fn="declick", workload=f"{a.minutes:g} min {ch}-ch {sr} Hz, {a.clicks} clicks",
        frames=n, hits=res.hits, raw=res.raw, kept=len(res.segs),
        declick_ms=dict(median=round(total_ms, 3), min=round(total_min, 3),
                        max=round(total_max, 3), runs=a.runs),
        bytes_moved=bytes_["total"], bytes_per_frame=round(bytes_["total"] / n, 2),
        stage_gbs=round(bytes_["total"] / (total_ms * 1e-3) / 1e9, 1),
        achievable_peak_gbs=round(copy_gbs, 1),
        frac_of_achievable_peak=round(bytes_["total"] / (total_ms * 1e-3) / 1e9 / copy_gbs, 3),
        passes_ms_sum=round(kernel_ms, 3),
        passes_frac_of_achievable_peak=round(
            sum(p["bytes"] for p in per_pass.values()) / (kernel_ms * 1e-3) / 1e9 / copy_gbs, 3),
        passes=per_pass,
        cpu_numpy_s=None if cpu_s is None else round(cpu_s, 3),
        cpu_how="tests/declick_ref.py, one core, same input",
        speedup=None if cpu_s is None else round(cpu_s * 1e3 / total_ms, 1),
        bit_identical_to_numpy=same)), flush=True)


if __name__ == "__main__":
    main()
