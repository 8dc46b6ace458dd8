#!/usr/bin/env python3
"""Generate ``tests/golden/compare_*.npz`` by running the REFERENCE script
``src/compare_audio.py`` itself (its ``find_delay_by_corr`` and its ``main``)
on the pairs of ``tests/golden/compare_cases.py``.

Build-container only, like ``tools/make_align_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for.  Nothing of the
reference is copied: a fixture holds the case, the SHA-256 of the regenerated
inputs, the delay (and, from tests/compare_ref.py's restatement, the arg-max k
behind it and the float64 margin of the correlation's top), and for the
``main`` cases the script's stdout, the columns of its CSV, the spectra its own
``stft_mag_avg`` returned (recorded by a wrapper around that function) and the
gain and SNR of the restatement, which is first checked to reproduce the
reference's CSV and stdout exactly.

Usage:  python tools/make_compare_goldens.py --ref /path/to/reference/src
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests import compare_ref  # noqa: E402
from tests.golden.compare_cases import (DELAY_CASES_FULL, ERROR_CASES, MAIN_CASES,  # noqa: E402
                                        MIN_MARGIN, SR, make_inputs)
from tests.golden_util import sha  # noqa: E402


def store(c):
    base, cand = make_inputs(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE["base.wav"] = (base, SR)
    sfstub.STORE["cand.wav"] = (cand, SR)
    return base, cand


def common(c, base, cand):
    return dict(in_sha=np.array([sha(base), sha(cand)]), meta=np.array(json.dumps(c)))


def delay_case(mod, c):
    base, cand = store(c)
    delay = mod.find_delay_by_corr(mod.power_mono(base), mod.power_mono(cand), SR)
    st = compare_ref.delay_estimate(base, cand, SR, 2000)
    assert st["delay"] == delay, (c["name"], st["delay"], delay)
    long_pair = len(base) > 20 * SR   # np.correlate on 80 000 x 80 000 lags: through the FFT
    s64 = compare_ref.delay_estimate(base, cand, SR, 2000, np.float64, fft64=long_pair)
    m64 = compare_ref.margin(s64["corr"])
    assert s64["k"] == st["k"] and m64 >= MIN_MARGIN, (c["name"], m64)
    print(f"{c['name']:22s} delay {delay:8d} k {st['k']:6d} nb {st['nb']:6d} margin {m64:.2e}")
    return dict(delay=np.array(delay, np.int64), k=np.array(st["k"], np.int64),
                nb=np.array(st["nb"], np.int64), margin64=np.array(m64), **common(c, base, cand))


def run_main(mod, c, tmp):
    """-> (stdout, csv columns, the spectra stft_mag_avg returned)."""
    spectra = []
    inner = mod.stft_mag_avg

    def recording(*a, **k):
        spectra.append(inner(*a, **k))
        return spectra[-1]

    buf = io.StringIO()
    cwd = os.getcwd()
    os.chdir(tmp)
    mod.stft_mag_avg = recording
    try:
        with contextlib.redirect_stdout(buf):
            mod.main("base.wav", "cand.wav", n_fft=c["n_fft"], hop=c["hop"])
    finally:
        mod.stft_mag_avg = inner
        os.chdir(cwd)
    with open(os.path.join(tmp, "diff_spectrum.csv")) as f:
        header = f.readline().rstrip("\n")
    cols = np.loadtxt(os.path.join(tmp, "diff_spectrum.csv"), delimiter=",", skiprows=1)
    return buf.getvalue(), header, cols, spectra


def main_case(mod, c, tmp):
    base, cand = store(c)
    text, header, cols, (b_mag, c_mag, c_mag2) = run_main(mod, c, tmp)
    n = compare_ref.main_numbers(base, cand, SR, c["n_fft"], c["hop"])
    assert compare_ref.report(n) == text, (compare_ref.report(n), text)
    assert np.array_equal(n["diff_db"].astype(np.float64), cols[:, 1])
    assert np.array_equal(n["b_mag"], b_mag) and np.array_equal(n["c_mag2"], c_mag2)
    st = compare_ref.delay_estimate(base, cand, SR, 2000)
    m64 = compare_ref.margin(compare_ref.delay_estimate(base, cand, SR, 2000, np.float64)["corr"])
    assert m64 >= MIN_MARGIN
    print(f"{c['name']:22s} delay {n['delay']:8d} gain {n['gain_db']:+.4f} dB "
          f"snr {n['snr_db']:.4f} dB")
    return dict(delay=np.array(n["delay"], np.int64), k=np.array(st["k"], np.int64),
                nb=np.array(st["nb"], np.int64), margin64=np.array(m64), stdout=np.array(text),
                header=np.array(header), freqs=cols[:, 0], diff_db=cols[:, 1].astype(np.float32),
                b_mag=b_mag, c_mag=c_mag, c_mag2=c_mag2, gain_db=np.array(n["gain_db"]),
                gain_lin=np.array(n["gain_lin"]), snr_db=np.array(n["snr_db"]),
                **common(c, base, cand))


def error_case(mod, c, tmp):
    base, cand = store(c)
    try:
        run_main(mod, c, tmp)
    except ValueError as e:
        print(f"{c['name']:22s} {e}")
        return dict(error=np.array(str(e)), **common(c, base, cand))
    raise AssertionError(c["name"] + ": the reference raised nothing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    mod = importlib.import_module("compare_audio")
    with tempfile.TemporaryDirectory() as tmp:
        for c in DELAY_CASES_FULL:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **delay_case(mod, c))
        for c in MAIN_CASES:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **main_case(mod, c, tmp))
        for c in ERROR_CASES:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"),
                                **error_case(mod, c, tmp))


if __name__ == "__main__":
    main()
