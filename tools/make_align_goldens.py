#!/usr/bin/env python3
"""Generate ``tests/golden/align_*.npz`` by running the REFERENCE script
``src/layer2_analyze_eq.py`` itself (its ``find_delay_by_corr`` and its
``main()``) on the pairs of ``tests/golden/align_cases.py``.

Build-container only, like ``tools/make_calib_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for, and matplotlib,
which runs on the Agg backend.  Nothing of the reference is copied: a fixture
holds the case, the SHA-256 of the regenerated inputs, the delay (and, from
tests/align_ref.py's restatement, the arg-max k behind it), the script's
stdout, the columns of its CSV, the medians its own ``stft_logpower_median``
returns on the aligned overlap, and the messages of its two error paths.

Usage:  python tools/make_align_goldens.py --ref /path/to/reference/src
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

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests import align_ref  # noqa: E402
from tests.golden.align_cases import (CLI_CASES, DELAY_CASES, ERROR_CASES, SR,  # noqa: E402
                                      make_pair)
from tests.golden_util import sha  # noqa: E402


def store(c):
    xt, xb = make_pair(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE["target.wav"] = (xt, SR)
    sfstub.STORE["base.wav"] = (xb, SR)
    return xt, xb


def run_main(mod, argv, tmp):
    """-> (stdout with the paths replaced, csv path, png path)."""
    csv, png = os.path.join(tmp, "curve.csv"), os.path.join(tmp, "curve.png")
    for p in (csv, png):
        if os.path.exists(p):
            os.remove(p)
    old = sys.argv
    sys.argv = ["layer2_analyze_eq.py", "--base", "base.wav", "--target", "target.wav",
                "--out_csv", csv, "--out_png", png] + list(argv)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            mod.main()
    finally:
        sys.argv = old
    return buf.getvalue().replace(csv, "{csv}").replace(png, "{png}"), csv, png


def delay_case(mod, c):
    xt, xb = store(c)
    delay = mod.find_delay_by_corr("target.wav", "base.wav", sr=SR, chunk_sec=c["chunk_sec"])
    st = align_ref.delay_estimate(xt, xb, SR, 2000, c["chunk_sec"])
    assert st["delay"] == delay, (c["name"], st["delay"], delay)
    m64 = align_ref.margin(align_ref.delay_estimate(xt, xb, SR, 2000, c["chunk_sec"],
                                                    np.float64)["corr"])
    print(f"{c['name']:20s} delay {delay:8d} k {st['k']:6d} margin {m64:.2e}")
    return dict(delay=np.array(delay, np.int64), k=np.array(st["k"], np.int64),
                margin64=np.array(m64), in_sha=np.array([sha(xt), sha(xb)]),
                meta=np.array(json.dumps(c)))


def cli_case(mod, c, tmp):
    xt, xb = store(c)
    text, csv, png = run_main(mod, c["argv"], tmp)
    cols = np.loadtxt(csv, delimiter=",", skiprows=1)
    assert os.path.getsize(png) > 0
    delay = mod.find_delay_by_corr("target.wav", "base.wav", sr=SR)
    st = align_ref.delay_estimate(xt, xb, SR, 2000, 25.0)
    assert st["delay"] == delay
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_fft", type=int, default=8192)
    ap.add_argument("--hop", type=int, default=4096)
    a, _ = ap.parse_known_args(c["argv"])
    bs, ts = max(0, -delay), max(0, delay)
    avail = min(len(xb) - bs, len(xt) - ts, int(6.0 * 60 * SR))
    _, med_b, used_b = mod.stft_logpower_median(xb[bs:bs + avail], SR, a.n_fft, a.hop, -65.0)
    _, med_t, used_t = mod.stft_logpower_median(xt[ts:ts + avail], SR, a.n_fft, a.hop, -65.0)
    print(f"{c['name']:20s} delay {delay:8d} used {used_b}/{used_t}")
    return dict(delay=np.array(delay, np.int64), k=np.array(st["k"], np.int64), stdout=np.array(text),
                freqs=cols[:, 0], delta_raw=cols[:, 1], delta_smooth=cols[:, 2],
                med_b=med_b, med_t=med_t, used=np.array([used_b, used_t], np.int64),
                in_sha=np.array([sha(xt), sha(xb)]), meta=np.array(json.dumps(c)))


def error_case(mod, c, tmp):
    xt, xb = store(c)
    try:
        run_main(mod, c["argv"], tmp)
    except ValueError as e:
        print(f"{c['name']:20s} {e}")
        return dict(error=np.array(str(e)), in_sha=np.array([sha(xt), sha(xb)]),
                    meta=np.array(json.dumps(c)))
    raise AssertionError(c["name"] + ": the reference raised nothing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    a = ap.parse_args()
    sys.path.insert(1, a.ref)
    mod = importlib.import_module("layer2_analyze_eq")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for c in DELAY_CASES:
            res[c["name"]] = delay_case(mod, c)
        for c in CLI_CASES:
            res[c["name"]] = cli_case(mod, c, tmp)
        for c in ERROR_CASES:
            res[c["name"]] = error_case(mod, c, tmp)
    for name, r in res.items():
        np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), **r)


if __name__ == "__main__":
    main()
