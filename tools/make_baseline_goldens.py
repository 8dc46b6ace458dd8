#!/usr/bin/env python3
"""Generate ``tests/golden/baseline_*.npz`` by running the REFERENCE script
``src/compare_to_baseline.py`` itself (its ``find_delay_by_corr``, its
``compute_metrics`` and its ``main``) on the cases of
``tests/golden/baseline_cases.py``.

Build-container only, like ``tools/make_compare_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for, and matplotlib,
which runs with ``MPLBACKEND=Agg``.  Nothing of the reference is copied: a
fixture holds the case, the SHA-256 of the regenerated inputs, and per candidate
the delay, the numbers ``compute_metrics`` returned (recorded by a wrapper
around that function), the four columns of its CSV as float32, the float64
margin of the correlation's top, and the error of the reference's float32
spectra against the float64 statement; per call the text of ``summary.txt`` and
stdout.  tests/baseline_ref.py's restatement is first checked to reproduce the
reference's CSV columns and ``summary.txt`` exactly.

Usage:  python tools/make_baseline_goldens.py --ref /path/to/reference/src
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

os.environ["MPLBACKEND"] = "Agg"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests import baseline_ref as br  # noqa: E402
from tests.golden.baseline_cases import (BASELINE_FILE, ERROR_CASES, MAIN_CASES,  # noqa: E402
                                         MIN_MARGIN, OUTDIR, SR, make_inputs)
from tests.golden_util import sha  # noqa: E402

BAND_KEYS = [k for k, _, _ in br.BANDS]


def store(c):
    base, cands = make_inputs(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE[BASELINE_FILE] = (base, SR)
    for k, x in zip(c["cands"], cands):
        sfstub.STORE[k["file"]] = (x, k.get("sr", SR))
    return base, cands


def argv_of(c):
    return ["--baseline", BASELINE_FILE, "--candidates", *[k["file"] for k in c["cands"]],
            "--outdir", OUTDIR, "--n_fft", str(c["n_fft"]), "--hop", str(c["hop"]),
            "--max_minutes", str(c["max_minutes"])]


def run_main(mod, c, tmp):
    """-> (stdout, summary.txt, per candidate (csv header, csv columns), the
    tuples compute_metrics returned, the delays find_delay_by_corr returned)."""
    metrics, delays = [], []
    inner_m, inner_d = mod.compute_metrics, mod.find_delay_by_corr

    def rec_m(*a, **k):
        metrics.append(inner_m(*a, **k))
        return metrics[-1]

    def rec_d(*a, **k):
        delays.append(inner_d(*a, **k))
        return delays[-1]

    buf = io.StringIO()
    cwd, argv = os.getcwd(), sys.argv
    os.chdir(tmp)
    mod.compute_metrics, mod.find_delay_by_corr = rec_m, rec_d
    sys.argv = ["compare_to_baseline.py"] + argv_of(c)
    try:
        with contextlib.redirect_stdout(buf):
            mod.main()
    finally:
        mod.compute_metrics, mod.find_delay_by_corr = inner_m, inner_d
        sys.argv = argv
        os.chdir(cwd)
    out = os.path.join(tmp, OUTDIR)
    with open(os.path.join(out, "summary.txt"), encoding="utf-8") as f:
        summary = f.read()
    csvs = []
    for k in c["cands"]:
        p = os.path.join(out, "diff_" + os.path.splitext(k["file"])[0] + ".csv")
        with open(p) as f:
            header = f.readline().rstrip("\n")
        csvs.append((header, np.loadtxt(p, delimiter=",", skiprows=1)))
    for png in ("delta_overlay.png", "env_rms_dbfs.png"):
        assert os.path.getsize(os.path.join(out, png)) > 0
    for p in os.listdir(out):
        os.remove(os.path.join(out, p))
    return buf.getvalue(), summary, csvs, metrics, delays


def main_case(mod, c, tmp):
    base, cands = store(c)
    files = [k["file"] for k in c["cands"]]
    text, summary, csvs, metrics, delays = run_main(mod, c, tmp)
    rs = br.run(base, cands, SR, c["n_fft"], c["hop"], c["max_minutes"])
    assert [r["delay"] for r in rs] == delays, (c["name"], delays)
    assert br.summary_text(BASELINE_FILE, files, rs, SR, c["max_minutes"]) == summary
    assert br.stdout_text(OUTDIR, files) == text, text
    r64 = br.run(base, cands, SR, c["n_fft"], c["hop"], c["max_minutes"], np.float64, delays)
    d = dict(in_sha=np.array([sha(base)] + [sha(x) for x in cands]), meta=np.array(json.dumps(c)),
             summary=np.array(summary), stdout=np.array(text), header=np.array(csvs[0][0]),
             n_cands=np.array(len(cands), np.int64))
    for i, (cand, r, q, m, (header, cols)) in enumerate(zip(cands, rs, r64, metrics, csvs)):
        assert header == br.CSV_HEADER
        assert np.array_equal(br.csv_columns(r).astype(np.float64), cols), (c["name"], i)
        assert (r["gain_db"], r["anchor"], r["snr"], r["noise_delta"]) == (m[4], m[5], m[9], m[8])
        assert r["stats"] == m[6] and r["music_err"] == float(m[7])
        assert mod.find_delay_by_corr(files[i], BASELINE_FILE, sr=SR) == r["delay"]
        s64 = br.find_delay(cand, base, SR, dtype=np.float64)
        m64 = br.margin(s64["corr"])
        assert s64["delay"] == r["delay"] and m64 >= MIN_MARGIN, (c["name"], i, m64)
        # the reference's float32 spectra against the float64 statement, in dB
        e32 = [float(np.max(np.abs(r[k].astype(np.float32).astype(np.float64) - q[k])))
               for k in ("Sb", "Sc")]
        smax = [float(np.max(np.abs(q[k]))) for k in ("Sb", "Sc")]
        print(f"{c['name']:22s} [{i}] delay {r['delay']:6d} margin {m64:.2e} gain "
              f"{r['gain_db']:+.4f} dB snr {r['snr']:.4f} dB music_err {r['music_err']:.4f} "
              f"e32 {e32[0]:.2e} {e32[1]:.2e} dB (spacing {np.spacing(np.float32(smax[0])):.2e})")
        d.update({f"delay_{i}": np.array(r["delay"], np.int64), f"margin64_{i}": np.array(m64),
                  f"cols_{i}": cols.astype(np.float32),
                  f"gain_db_{i}": np.array(m[4]), f"anchor_{i}": np.array(m[5]),
                  f"snr_{i}": np.array(m[9]), f"music_err_{i}": np.array(float(m[7])),
                  f"noise_delta_{i}": np.array(m[8]),
                  f"stats_{i}": np.array([m[6][k] for k in BAND_KEYS]),
                  f"e32_{i}": np.array(e32), f"smax_{i}": np.array(smax)})
        assert np.array_equal(d[f"cols_{i}"].astype(np.float64), cols)  # float32 throughout
    return d


def error_case(mod, c, tmp):
    base, cands = store(c)
    try:
        run_main(mod, c, tmp)
    except ValueError as e:
        print(f"{c['name']:22s} {e}")
        return dict(error=np.array(str(e)), meta=np.array(json.dumps(c)),
                    in_sha=np.array([sha(base)] + [sha(x) for x in cands]))
    raise AssertionError(c["name"] + ": the reference raised nothing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    mod = importlib.import_module("compare_to_baseline")
    with tempfile.TemporaryDirectory() as tmp:
        for c in MAIN_CASES:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **main_case(mod, c, tmp))
        for c in ERROR_CASES:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"),
                                **error_case(mod, c, tmp))
        # find_delay_by_corr on its own: the rate check's own message
        c = ERROR_CASES[-1]
        store(c)
        try:
            mod.find_delay_by_corr(c["cands"][0]["file"], BASELINE_FILE, sr=SR)
        except ValueError as e:
            fx = dict(np.load(os.path.join(OUT_DIR, c["name"] + ".npz")))
            fx["error_find_delay"] = np.array(str(e))
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **fx)
            print(f"{c['name']:22s} {e}")


if __name__ == "__main__":
    main()
