#!/usr/bin/env python3
"""Output bits of the analysis spectrum entry points (``tm_analysis.hip``), for
comparing two builds of the library: prints one line ``case sha256(output
bytes)`` per case for the library ``TOMATIS_HIP_LIB`` names (default: the one in
the tree) and asserts nothing.  A case is an entry point at one n_fft and hop:
its digest runs over the return codes and output bytes of every frame count and
every variant (modes, channels, anchors, bands, frame lists) in a fixed order;
``--each`` prints a line per call instead, to find the one that differs.  Two
builds compute the same bits when their listings are identical files:

  python -m tomatis_audio_processor_amd.build --out /path/libtomatis_parent.so   # in a worktree
  TOMATIS_HIP_LIB=/path/libtomatis_parent.so python tools/an_bits.py > parent.txt
  python tools/an_bits.py > new.txt && cmp parent.txt new.txt

The entry points are called directly, so the Python of this tree does not
matter.  Needs an MI355X; run each library in a fresh process.

Cases: the smallest shapes at which each path can go wrong.  n_fft 16 (one bin
per thread), 18 (Bluestein, M = 64), 256, 1000 (Bluestein), 2048, 3001 (odd: no
n/2 bin), 8191 (odd, Bluestein, M = 16384), 16384; hop n_fft // 4 and once
n_fft; frame counts 1 (a pair kernel's block without a second frame), 2, 7, 17
(nine pairs: two slabs of 8, the last pair unpartnered), 35 (three slabs of 16
frames), at M = 16384 at most 3.  Inputs are seeded and every signal has a
non-zero mean, so bin n/2 lies far under bin 0.  Hashing bytes covers NaN.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FFTS = (16, 18, 256, 1000, 2048, 3001, 8191, 16384)
FRAMES = (1, 2, 7, 17, 35)
LEVEL_N = (256, 8192, 16, 1000, 16384)   # tree sizes, then pairwise-program sizes
MEAN_WIN = (16, 1000, 4800)              # tomatis_an_frame_power_mean windows


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("an_bits needs the MI355X")
    from tomatis_audio_processor_amd import _lib
    from tomatis_audio_processor_amd._lib import lib, ptr, stream_handle
    L, hs = lib(), stream_handle()
    print(f"# library: {os.path.basename(_lib.lib_path())}", file=sys.stderr)

    each = "--each" in sys.argv[1:]
    digests = {}  # case -> running sha256, in first-use order

    def show(call, rc, *outs):
        """``call`` is "entry/variant n_fft=.. hop=.. F=..": the case is the entry
        point with n_fft and hop."""
        torch.cuda.synchronize()
        name, shape = call.split(" ", 1)
        case = name.split("/")[0] + " " + shape.rsplit(" ", 1)[0]
        h = hashlib.sha256() if each else digests.setdefault(case, hashlib.sha256())
        if rc != 0:
            print(f"# {call}: status {rc}", file=sys.stderr)
        h.update(f"{call} rc={rc}".encode())
        for o in outs:
            h.update(o.cpu().numpy().tobytes())
        if each:
            print(f"{call} rc={rc} {h.hexdigest()}")

    def new(shape, dtype=torch.float32):
        return torch.full(shape, -7.0, dtype=dtype, device="cuda")

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    for n_fft in N_FFTS:
        big = n_fft > 4096                      # M = 16384
        hops = (n_fft // 4, n_fft) if n_fft == 256 else (n_fft // 4,)
        for hop in hops:
            for F in ((1, 2, 3) if big else FRAMES):
                rng = np.random.default_rng(1000 * n_fft + 10 * F + (hop == n_fft))
                n = n_fft + (F - 1) * hop + hop // 2
                xs = dev(0.2 * rng.standard_normal((n, 2)) + 0.05)
                ys = dev(0.1 * rng.standard_normal((n, 2)) + 0.5 * xs.cpu().numpy() + 0.02)
                xm, ym = xs[:, 0].contiguous(), ys[:, 0].contiguous()
                win = dev(np.hanning(n_fft) + 0.01)
                nb = n_fft // 2 + 1
                tag = f"n_fft={n_fft} hop={hop} F={F}"
                anchors = ((0, 0), (3, 4), (0, nb))
                bands = ((0, 0, 0, 0), (1, nb // 2 + 1, nb // 4, nb), (0, nb, 0, nb))

                for kind, kname in ((0, "MAG"), (1, "LOGPOW")):
                    for sig, x, ch in ((0, xm, 1), (1, xs, 2)):
                        out = new((F, nb))
                        rc = L.tomatis_an_spectra(ptr(x), None, n, ch, n_fft, hop, kind, sig,
                                                  C.c_float(0.75), ptr(win), ptr(out), hs)
                        show(f"spectra/{kname}/sig{sig} {tag}", rc, out)
                for ch, x, y in ((1, xm, ym), (2, xs, ys)):
                    out = new((F, nb))
                    rc = L.tomatis_an_spectra(ptr(x), ptr(y), n, ch, n_fft, hop, 2, 0,
                                              C.c_float(1.0), ptr(win), ptr(out), hs)
                    show(f"spectra/RATIO/ch{ch} {tag}", rc, out)
                    for a in anchors:
                        rows = new((F, nb))
                        rc = L.tomatis_an_anchored_ratio(ptr(x), ptr(y), n, ch, n_fft, hop, *a,
                                                         ptr(win), ptr(rows), hs)
                        show(f"anchored_ratio/ch{ch}/a{a[0]}-{a[1]} {tag}", rc, rows)
                    for b in bands:
                        be = new((F, 4))
                        rc = L.tomatis_an_pair_band_energy(ptr(x), ptr(y), n, ch, n_fft, hop, *b,
                                                           ptr(win), ptr(be), hs)
                        show(f"pair_band_energy/ch{ch}/b{'-'.join(map(str, b))} {tag}", rc, be)
                    for a, b in zip(anchors, bands):
                        rows, be = new((F, nb)), new((F, 4))
                        rc = L.tomatis_an_verify_pair(ptr(x), ptr(y), n, ch, n_fft, hop, *a, *b,
                                                      ptr(win), ptr(rows), ptr(be), hs)
                        show(f"verify_pair/ch{ch}/a{a[0]}-{a[1]}/b{'-'.join(map(str, b))} {tag}",
                             rc, rows, be)
                for b in bands:
                    out = new((F, 2))
                    rc = L.tomatis_an_band_energy(ptr(xs), n, n_fft, hop, *b, ptr(win), ptr(out), hs)
                    show(f"band_energy/b{'-'.join(map(str, b))} {tag}", rc, out)
                for sig, x, ch in ((0, xm, 1), (1, xs, 2)):
                    work = new((max(1, int(L.tomatis_an_spectrum_mean_work_doubles(F, nb))),),
                               torch.float64)
                    out = new((nb,), torch.float64)
                    rc = L.tomatis_an_spectrum_mean(ptr(x), n, ch, n_fft, hop, sig, C.c_float(0.75),
                                                    ptr(win), ptr(work), ptr(out), hs)
                    show(f"spectrum_mean/sig{sig} {tag}", rc, out)
                for b in bands:
                    for want_rows in (False, True):
                        means = new((F, 2), torch.float64)
                        rows = new((F, nb)) if want_rows else None
                        rc = L.tomatis_an_pair_tilt(ptr(xs), ptr(ys), n, n_fft, hop, *b, ptr(win),
                                                    ptr(rows), ptr(means), hs)
                        show(f"pair_tilt/rows{int(want_rows)}/b{'-'.join(map(str, b))} {tag}", rc,
                             means, *([rows] if want_rows else []))
                lists = (("all", None), ("third", np.arange(0, F, 3, dtype=np.int32)),
                         ("one", np.array([F - 1], np.int32)), ("empty", np.zeros(0, np.int32)))
                for lname, fl in lists:
                    n_sel = F if fl is None else len(fl)
                    buf = None if fl is None else np.ascontiguousarray(
                        fl if len(fl) else np.zeros(1, np.int32))  # an empty list, not NULL
                    work = new((max(1, int(L.tomatis_an_pair_diff_mean_work_doubles(n_sel, nb))),),
                               torch.float64)
                    out = new((nb,), torch.float64)
                    rc = L.tomatis_an_pair_diff_mean(
                        ptr(xs), ptr(ys), n, n_fft, hop, ptr(win),
                        None if buf is None else buf.ctypes.data_as(C.c_void_p), n_sel, ptr(work),
                        ptr(out), hs)
                    show(f"pair_diff_mean/{lname} {tag}", rc, out)

    # levels: tomatis_an_frame_r (perfect tree / pairwise program) and frame_power_mean
    for n_fft in LEVEL_N:
        hop = n_fft // 4
        for F in ((1, 3) if n_fft > 4096 else (1, 7)):
            rng = np.random.default_rng(77 * n_fft + F)
            n = n_fft + (F - 1) * hop + hop // 2
            xs = dev(0.2 * rng.standard_normal((n, 2)) + 0.05)
            xm = xs[:, 0].contiguous()
            for mode, x, ch in ((0, xm, 1), (0, xs, 2), (1, xs, 2)):
                r = new((F,))
                rc = L.tomatis_an_frame_r(ptr(x), n, ch, n_fft, hop, mode, C.c_float(0.75), ptr(r),
                                          hs)
                show(f"frame_r/mode{mode}/ch{ch} n_fft={n_fft} hop={hop} F={F}", rc, r)
    for w in MEAN_WIN:
        hop, F = w // 2, 9
        rng = np.random.default_rng(5 * w)
        n = w + (F - 1) * hop + 1
        xs = dev(0.2 * rng.standard_normal((n, 2)) + 0.05)
        out = new((F,))
        rc = L.tomatis_an_frame_power_mean(ptr(xs), n, w, hop, ptr(out), hs)
        show(f"frame_power_mean win={w} hop={hop} F={F}", rc, out)
    for case, h in digests.items():
        print(f"{case} {h.hexdigest()}")


if __name__ == "__main__":
    main()
