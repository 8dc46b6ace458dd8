#!/usr/bin/env python3
"""Time of the parameter-recovery tools on the device on
one MI355X, on a device-resident 30-minute 48 kHz stereo input / output pair at
4096 / 2048 (the two scripts' constants; the pair is tools/bench_verify.py's):

  (a) tomatis_an_pair_tilt without rows: one transform per frame, 16 bytes out;
  (b) the same with the rows stored;
  (c) tomatis_an_pair_diff_mean over all frames;
  (d) tomatis_an_verify_pair on the same pair (the yardstick: two transforms per
      frame and the rows stored);
  (e) the unfused composition of (a): two TOMATIS_AN_MAG spectrograms of the
      power monos, then torch elementwise ops and two means per frame;
  (f) ``reverse_engineer_params.analyze`` and ``verify_tilt_amplitude.analyze``
      end to end on the resident pair (delay estimate, levels, kernels, the host
      statistics and the printed text; no files).

Prints one JSON line.

Method: HIP events on the library's stream, warm-up, (a) to (e) alternating in
one loop, median / min / max of ``--runs`` (>= 20) calls each.  The region is
the launch or launches and the allocation of the outputs from torch's caching
allocator, and for (a) to (c) the window's upload inside the wrapper: a call's
time on the stream, not a profiler's kernel time.  (f) is host wall time around
a run that ends in device read-backs, median of ``--e2e_runs``.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--n_fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--e2e_runs", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverse needs the MI355X: there is nothing to time without it")
    from tomatis_audio_processor_amd import analysis as A
    from tomatis_audio_processor_amd import engine as E
    from tomatis_audio_processor_amd import reverse_engineer_params as rev
    from tomatis_audio_processor_amd import verify_tilt_amplitude as amp
    from tools.bench_verify import make_pair

    sr = 48000
    n = int(a.minutes * 60 * sr)
    x, y = make_pair(torch, E, n, sr, a.n_fft, a.hop)
    freqs = np.fft.rfftfreq(a.n_fft, 1 / sr)
    lo, hi = rev.band_range(freqs, *rev.LOW_BAND), rev.band_range(freqs, *rev.HIGH_BAND)
    anchor = A.band_bins(freqs, 900, 1100)
    vbands = (*A.band_bins(freqs, 200, 1000), *A.band_bins(freqs, 2000, 8000))
    F = A._n_frames(n, a.n_fft, a.hop)
    nb = a.n_fft // 2 + 1
    win = torch.from_numpy(np.hanning(a.n_fft).astype(np.float32)).cuda()
    eps = 1e-12

    def tilt():
        return A.pair_tilt(x, y, a.n_fft, a.hop, lo, hi)

    def tilt_rows():
        return A.pair_tilt(x, y, a.n_fft, a.hop, lo, hi, want_rows=True)

    def diff_mean():
        return A.pair_diff_mean(x, y, a.n_fft, a.hop)

    def verify_pair():
        return A.verify_spectra(x, y, a.n_fft, a.hop, anchor=anchor, bands=vbands, fused=True,
                                win=win)

    def unfused():
        ma = A._spectra(x, None, n, 2, a.n_fft, a.hop, A.AN_MAG, A.AN_SIG_POWER_MONO)
        mb = A._spectra(y, None, n, 2, a.n_fft, a.hop, A.AN_MAG, A.AN_SIG_POWER_MONO)
        d = 20.0 * torch.log10(mb + eps) - 20.0 * torch.log10(ma + eps)
        return torch.stack([d[:, lo[0]:lo[1]].double().mean(dim=1),
                            d[:, hi[0]:hi[1]].double().mean(dim=1)], dim=1)

    fns = dict(pair_tilt=tilt, pair_tilt_rows=tilt_rows, pair_diff_mean=diff_mean,
               verify_pair=verify_pair, unfused=unfused)
    m1, _ = tilt()
    m2 = unfused()
    torch.cuda.synchronize()
    agree = float((m1 - m2).abs().max())
    del m1, m2
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(max(20, a.runs)):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            t[name].append(e0.elapsed_time(e1))

    def stats(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4),
                    max_ms=round(max(v), 4))

    e2e = {"reverse_engineer_params": [], "verify_tilt_amplitude": []}
    res = {}
    for name, fn in (("reverse_engineer_params", rev.analyze), ("verify_tilt_amplitude", amp.analyze)):
        for i in range(a.e2e_runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                res[name] = fn(x, y, sr=sr, n_fft=a.n_fft, hop=a.hop)
            torch.cuda.synchronize()
            if i:  # the first run warms up
                e2e[name].append((time.perf_counter() - t0) * 1e3)

    med = {k: statistics.median(v) for k, v in t.items()}
    pcm_bytes = 2 * (a.n_fft / a.hop) * n * 2 * 4
    print(json.dumps(dict(
        what="reverse_engineer_params / verify_tilt_amplitude on the device", minutes=a.minutes,
        n_fft=a.n_fft, hop=a.hop, frames=F, bins=nb,
        **{k: stats(v) for k, v in t.items()},
        pair_tilt_over_verify_pair=round(med["pair_tilt"] / med["verify_pair"], 3),
        pair_tilt_over_unfused=round(med["pair_tilt"] / med["unfused"], 3),
        pair_diff_mean_over_verify_pair=round(med["pair_diff_mean"] / med["verify_pair"], 3),
        pair_tilt_algorithmic_GBps=round(pcm_bytes / (med["pair_tilt"] * 1e-3) / 1e9, 1),
        unfused_max_abs_difference_db=agree,
        e2e_ms={k: stats(v) for k, v in e2e.items()},
        delay=res["reverse_engineer_params"]["delay"],
        amplitude_classes=[res["verify_tilt_amplitude"]["n_c1"],
                           res["verify_tilt_amplitude"]["n_c2"]])))


if __name__ == "__main__":
    main()
