#!/usr/bin/env python3
"""Time of compare_to_baseline on the device on one MI355X,
on a device-resident 8-minute 48 kHz stereo baseline and three candidates at
4096 / 2048 (the reference's defaults):

  (a) the fused mean log-power spectrum, tomatis_an_spectrum_mean (one launch and
      the fold over slabs);
  (b) the composition the library had before it, in the same process:
      tomatis_an_spectra(LOGPOW) into a [F, n_bins] float32 spectrogram, then
      tomatis_an_frame_mean (a float32 mean: (b) is the time of that data flow,
      not the same number);
  (c) ``compare_to_baseline.compare_many`` with the three candidates end to end:
      delays, overlaps, metrics, CSVs, summary.txt and both plots;

next to the time of the reference's own arithmetic for ONE candidate on one core
of this machine (tests/baseline_ref.py's restatement of it: resample_poly +
fftconvolve for the delay, two frame-by-frame numpy STFTs, the time-domain sums;
without reading the files, which the reference does four times per candidate).
Prints one JSON line.

Method: HIP events on the library's stream, warm-up, (a) and (b) alternating in
one loop, median / min / max of ``--runs`` (>= 20) calls each; (c) is host wall
time around a run that ends in a synchronise, median of ``--e2e_runs``.  The
fused kernel's algorithmic bytes are the PCM read once per hop overlap (n_fft /
hop times 8 B per stereo sample) plus the slab rows written and read, set
against the copy bandwidth ``tomatis_copy_probe`` reaches in the same process.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHIFTS = (777, -3210, 123456)
GAINS = (0.7, 0.9, 0.5)


def make_set(torch, n, seed):
    """-> (base, [cand, ...]): noise under a random 50 Hz amplitude contour; each
    candidate plays the base's material ``shift`` samples later, scaled, tilted by
    a two-tap filter and mixed with a little noise of its own."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pad = max(abs(s) for s in SHIFTS) + 1
    m = n + 2 * pad
    amp = 0.02 + 0.3 * torch.rand((m // 960 + 2,), generator=g, device="cuda")
    amp = torch.repeat_interleave(amp, 960)[:m].reshape(m, 1)
    u = torch.randn((m, 2), generator=g, device="cuda", dtype=torch.float32)
    u.mul_(amp).clamp_(-1.0, 1.0)
    base = u[pad:pad + n].clone()     # an allocation of its own: 16-byte aligned
    cands = []
    for shift, gain in zip(SHIFTS, GAINS):
        a = u[pad - shift:pad - shift + n]
        b = u[pad - shift - 1:pad - shift - 1 + n]
        own = torch.randn((n, 2), generator=g, device="cuda", dtype=torch.float32)
        cands.append((gain * a + 0.2 * gain * b + 0.01 * own).contiguous())
    return base, cands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--n_fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e_runs", type=int, default=5)
    ap.add_argument("--no_cpu", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import ctypes as C
    import torch
    from tomatis_audio_processor_amd import analysis, compare_to_baseline as cb, dsp
    from tomatis_audio_processor_amd._lib import check, lib, ptr, stream_handle
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare_to_baseline needs an MI355X: there is no CPU fallback")
    h, st = lib(), stream_handle()

    sr, n_fft, hop = a.sr, a.n_fft, a.hop
    n = int(a.minutes * 60 * sr)
    base, cands = make_set(torch, n, 778)
    F = analysis._n_frames(n, n_fft, hop)
    nb = n_fft // 2 + 1

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                    max=round(max(ms), 4), runs=len(ms))

    flat = base.reshape(-1)
    cp_src = flat[: flat.numel() // 4 * 4]
    cp_dst = torch.empty_like(cp_src)
    probe = lambda: check(h.tomatis_copy_probe(ptr(cp_src), ptr(cp_dst), cp_src.numel(), st),  # noqa: E731
                          "copy_probe")
    for _ in range(a.warmup):
        probe()
    cp_ms = statistics.median([event_ms(probe) for _ in range(a.runs)])
    copy_gbs = 2.0 * 4.0 * cp_src.numel() / (cp_ms * 1e-3) / 1e9
    del cp_dst

    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    slabs_doubles = int(h.tomatis_an_spectrum_mean_work_doubles(F, nb))
    work = torch.empty(slabs_doubles, dtype=torch.float64, device="cuda")
    out64 = torch.empty(nb, dtype=torch.float64, device="cuda")
    spec = torch.empty((F, nb), dtype=torch.float32, device="cuda")
    out32 = torch.empty(nb, dtype=torch.float32, device="cuda")
    one = C.c_float(1.0)
    PM, LOGPOW = analysis.AN_SIG_POWER_MONO, analysis.AN_LOGPOW

    def fused():
        check(h.tomatis_an_spectrum_mean(ptr(base), n, 2, n_fft, hop, PM, one, ptr(win), ptr(work),
                                         ptr(out64), st), "an_spectrum_mean")

    def composed():
        check(h.tomatis_an_spectra(ptr(base), None, n, 2, n_fft, hop, LOGPOW, PM, one, ptr(win),
                                   ptr(spec), st), "an_spectra")
        check(h.tomatis_an_frame_mean(ptr(spec), F, nb, ptr(out32), st), "an_frame_mean")

    def spectra_only():
        check(h.tomatis_an_spectra(ptr(base), None, n, 2, n_fft, hop, LOGPOW, PM, one, ptr(win),
                                   ptr(spec), st), "an_spectra")

    for _ in range(a.warmup):
        fused(), composed()
    torch.cuda.synchronize()
    ms_a, ms_b, ms_s = [], [], []
    for _ in range(a.runs):          # alternating: both see the same neighbours
        ms_a.append(event_ms(fused))
        ms_b.append(event_ms(composed))
        ms_s.append(event_ms(spectra_only))
    # the two agree as a float64 mean and a float32 mean of the same float32 values do
    agree = float((out64 - out32.double()).abs().max().item())
    fused_bytes = 8 * n * (n_fft // hop) + 2 * 8 * slabs_doubles + 8 * nb
    med_a = statistics.median(ms_a)

    sums = torch.empty(3075, dtype=torch.float64, device="cuda")
    m = min(base.shape[0], cands[0].shape[0])
    ms_sum = [event_ms(lambda: check(h.tomatis_cmp_mono_sums(ptr(base), ptr(cands[0]), m, one,
                                                             ptr(sums), st), "cmp_mono_sums"))
              for _ in range(a.warmup + a.runs)][a.warmup:]

    names = [f"cand{i}" for i in range(len(cands))]
    e2e, parts = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        def run_many():
            with contextlib.redirect_stdout(io.StringIO()):
                r = cb.compare_many(base, cands, tmp, sr, n_fft, hop, a.minutes, names=names)
            torch.cuda.synchronize()
            return r
        results = run_many()
        for _ in range(a.e2e_runs):
            t0 = time.perf_counter()
            run_many()
            e2e.append((time.perf_counter() - t0) * 1e3)
        # the same without the files: delay, overlap and metrics of the three candidates
        t0 = time.perf_counter()
        for c in cands:
            b2, c2, _ = cb.get_aligned_overlap(base, c, sr, a.minutes)
            cb.compute_metrics(b2, c2, sr, n_fft, hop)
        torch.cuda.synchronize()
        parts["metrics_only_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        t0 = time.perf_counter()
        cb._plots(tmp, results, sr)
        parts["plots_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

    cpu_s, cpu_delay = None, None
    if not a.no_cpu:
        from tests import baseline_ref as br
        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # one core
        except (AttributeError, OSError):
            pass
        hb, hc = base.cpu().numpy(), cands[0].cpu().numpy()
        t0 = time.perf_counter()
        r = br.run(hb, [hc], sr, n_fft, hop, a.minutes)[0]
        cpu_s = time.perf_counter() - t0
        cpu_delay = r["delay"]

    print(json.dumps(dict(
        fn="compare_to_baseline", workload=f"{a.minutes:g} min stereo {sr} Hz, {n_fft}/{hop}, "
        f"{len(cands)} candidates", frames=F, n_bins=nb, slab_rows=slabs_doubles // nb,
        achievable_peak_gbs=round(copy_gbs, 1),
        a_fused_ms=stats(ms_a), b_composed_ms=stats(ms_b), b_spectra_only_ms=stats(ms_s),
        a_over_b=round(med_a / statistics.median(ms_b), 3),
        a_bytes=fused_bytes, a_gbs=round(fused_bytes / (med_a * 1e-3) / 1e9, 1),
        a_frac_of_copy=round(fused_bytes / (med_a * 1e-3) / 1e9 / copy_gbs, 3),
        a_vs_b_max_abs_db=agree, mono_sums_ms=stats(ms_sum),
        c_compare_many_ms=stats(e2e), c_parts=parts,
        delays=[r["delay"] for r in results],
        music_err=[round(float(r["music_err"]), 4) for r in results],
        cpu_one_candidate_s=None if cpu_s is None else round(cpu_s, 3), cpu_delay=cpu_delay,
        cpu_how="tests/baseline_ref.run (the reference's numpy / scipy arithmetic), one "
                "candidate, one core, arrays in memory")), flush=True)


if __name__ == "__main__":
    main()
