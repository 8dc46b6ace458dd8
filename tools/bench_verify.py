#!/usr/bin/env python3
"""Time of the acceptance validator on the device on one
MI355X, on a device-resident 30-minute 48 kHz stereo input / output pair at
4096 / 2048 (the reference's defaults):

  (a) sections C and D's spectra fused: tomatis_an_verify_pair, one launch, one
      transform per (frame, channel) for the anchored rows and the band sums;
  (b) the same from two launches: tomatis_an_anchored_ratio, then
      tomatis_an_pair_band_energy (the bits are the same, checked here);
  (c) ``verify_tomatis_15db_v2.verify`` end to end on the resident pair: peak,
      DC, levels, the threshold bisection, spectra, two medians, tilt index, the
      report text (no files, no plots);

next to the time of the reference's own arithmetic on one core of this machine
(tests/verify_ref.py's restatement, frame-vectorised numpy, on the first
``--ref_seconds`` of the same pair; the reference itself loops over frames in
Python and is slower).  Prints one JSON line.

Method: HIP events on the library's stream, warm-up, (a) and (b) alternating in
one loop, median / min / max of ``--runs`` (>= 20) calls each.  The window is
resident and outside the timed region; the region is the launch (two for (b))
and the allocation of its outputs from torch's caching allocator, no copy: a
call's time on the stream, not a profiler's kernel time.  (c) is host wall
time around a run that ends in device read-backs, median of ``--e2e_runs``.
Algorithmic bytes of (a): both PCM streams read once per hop overlap (n_fft /
hop times), the rows written once.
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


def make_pair(torch, E, n, sr, n_fft, hop):
    """The synthetic stream re-enveloped to -30 / -50 dBFS halves and this
    build's own +-15 dB output of it (linear gate at -40 dBFS, hysteresis 1 dB,
    no up-delay), both resident."""
    ss = E.StreamSet.synthetic(1, n, 2, sr, seed0=1000)
    idx = torch.arange(n, device=ss.x.device)
    ph = torch.remainder(idx, 3 * sr)
    g = torch.where((ph >= sr // 100) & (ph < (3 * sr) // 2),
                    torch.tensor(10.0 ** (10 / 20), device=ss.x.device),
                    torch.tensor(10.0 ** (-10 / 20), device=ss.x.device)).to(torch.float32)
    x = (ss.x[:n * 2].view(n, 2) * g[:, None]).contiguous()
    del idx, ph, g
    ss2 = E.StreamSet(x=x.reshape(-1), offs=[0], lens=[n], ch=2, sr=sr)
    pipe = E.GatePipeline(ss2, gate_ui=50, gate_mode="linear", gate_scale=1.0, gate_offset=-90.0,
                          hysteresis_db=1.0, up_delay_ms=0.0, n_fft=n_fft, hop=hop)
    res = pipe.run()
    torch.cuda.synchronize()
    y = res.y[:n * 2].view(n, 2).clone()
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--n_fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--e2e_runs", type=int, default=5)
    ap.add_argument("--ref_seconds", type=float, default=120.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify needs the MI355X: there is nothing to time without it")
    from tomatis_audio_processor_amd import analysis as A
    from tomatis_audio_processor_amd import engine as E
    from tomatis_audio_processor_amd import verify_tomatis_15db_v2 as v2
    from tests import verify_ref as vr

    sr = 48000
    n = int(a.minutes * 60 * sr)
    x, y = make_pair(torch, E, n, sr, a.n_fft, a.hop)
    freqs = np.fft.rfftfreq(a.n_fft, 1 / sr)
    anchor = A.band_bins(freqs, 900, 1100)
    bands = (*A.band_bins(freqs, 200, 1000), *A.band_bins(freqs, 2000, 8000))
    F = A._n_frames(n, a.n_fft, a.hop)
    nb = a.n_fft // 2 + 1

    win = torch.from_numpy(np.hanning(a.n_fft).astype(np.float32)).cuda()

    def fused():
        return A.verify_spectra(x, y, a.n_fft, a.hop, anchor=anchor, bands=bands, fused=True,
                                win=win)

    def split():
        return A.verify_spectra(x, y, a.n_fft, a.hop, anchor=anchor, bands=bands, fused=False,
                                win=win)

    r1, b1 = fused()
    r2, b2 = split()
    torch.cuda.synchronize()
    same = bool(torch.equal(r1, r2) and torch.equal(b1, b2))
    del r1, r2, b1, b2
    t = {"fused": [], "split": []}
    for _ in range(3):
        fused(), split()
    torch.cuda.synchronize()
    for _ in range(max(20, a.runs)):
        for name, fn in (("fused", fused), ("split", split)):
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

    e2e = []
    kw = dict(n_fft=a.n_fft, hop=a.hop, out_prefix=None, plots=False)
    R = None
    for i in range(a.e2e_runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            R = v2.verify(x, y, sr, **kw)
        torch.cuda.synchronize()
        if i:  # the first run warms up
            e2e.append((time.perf_counter() - t0) * 1e3)

    # the reference's arithmetic (numpy restatement) on one core, on a slice
    m = min(n, int(a.ref_seconds * sr))
    xs, ys = x[:m].cpu().numpy(), y[:m].cpu().numpy()
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    Rr = vr.run_v2(xs, ys, sr, dict(hyst_db=1.0, up_delay_ms=0, target_c2=0.5, fc=1000, slope=12,
                                    c1_low=15.0, c1_high=-15.0, c2_low=-15.0, c2_high=15.0,
                                    n_fft=a.n_fft, hop=a.hop, level_percentile=10))
    ref_s = time.perf_counter() - t0

    pcm_bytes = 2 * (a.n_fft / a.hop) * n * 2 * 4
    row_bytes = F * nb * 4
    med = statistics.median(t["fused"])
    print(json.dumps(dict(
        what="verify_tomatis_15db_v2 on the device", minutes=a.minutes, n_fft=a.n_fft, hop=a.hop,
        frames=F, fused=stats(t["fused"]), split=stats(t["split"]), fused_equals_split=same,
        fused_algorithmic_GBps=round((pcm_bytes + row_bytes) / (med * 1e-3) / 1e9, 1),
        verify_e2e_ms=stats(e2e), verify_exit_code=R["exit_code"],
        verify_T=round(float(R["optimal_T"]), 4), verify_used=[R["c1_n"], R["c2_n"]],
        ref_numpy_seconds=round(ref_s, 3), ref_numpy_audio_seconds=m / sr,
        ref_numpy_extrapolated_s=round(ref_s * n / m, 1), ref_exit_code=int(not Rr["ok"]))))


if __name__ == "__main__":
    main()
