#!/usr/bin/env python3
"""Generate ``tests/golden/rational_*.npz`` by running the REFERENCE's two delay
estimates themselves, ``src/layer2_analyze_eq.py``'s ``find_delay_by_corr``
("valid" correlation of the middle chunk) and ``src/compare_audio.py``'s
("full" correlation of the whole envelopes), on the 44.1 kHz, 88.2 kHz and
192 kHz pairs of ``tests/golden/rational_cases.py``.

Build-container only, like ``tools/make_align_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for, and matplotlib,
which runs on the Agg backend.  Nothing of the reference is copied: a fixture
holds the case, the SHA-256 of the regenerated inputs, the two delays and, from
the restatements tests/align_ref.py and tests/compare_ref.py (first checked to
give the reference's delay), the arg-max k behind each, the base envelope's
length nb and the float64 margin of each correlation's top, which must be at
least MIN_MARGIN.

Usage:  python tools/make_rational_goldens.py --ref /path/to/reference/src
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests import align_ref, compare_ref  # noqa: E402
from tests.golden.rational_cases import DS_SR, MIN_MARGIN, RATIONAL_CASES, make_pair  # noqa: E402
from tests.golden_util import sha  # noqa: E402


def case(l2, ca, c):
    sr = c["sr"]
    xt, xb = make_pair(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE["target.wav"] = (xt, sr)
    sfstub.STORE["base.wav"] = (xb, sr)
    # layer2_analyze_eq / calibrate_to_baseline_v2: target against the base's middle chunk
    delay = l2.find_delay_by_corr("target.wav", "base.wav", sr=sr, chunk_sec=c["chunk_sec"])
    st = align_ref.delay_estimate(xt, xb, sr, DS_SR, c["chunk_sec"])
    assert st["delay"] == delay, (c["name"], st["delay"], delay)
    s64 = align_ref.delay_estimate(xt, xb, sr, DS_SR, c["chunk_sec"], np.float64)
    m64 = align_ref.margin(s64["corr"])
    assert (s64["k"], s64["delay"]) == (st["k"], delay) and m64 >= MIN_MARGIN, (c["name"], m64)
    # compare_audio: the candidate (target) against the base, whole envelopes
    delay_f = ca.find_delay_by_corr(ca.power_mono(xb), ca.power_mono(xt), sr)
    sf = compare_ref.delay_estimate(xb, xt, sr, DS_SR)
    assert sf["delay"] == delay_f, (c["name"], sf["delay"], delay_f)
    f64 = compare_ref.delay_estimate(xb, xt, sr, DS_SR, np.float64)
    mf64 = compare_ref.margin(f64["corr"])
    assert (f64["k"], f64["delay"]) == (sf["k"], delay_f) and mf64 >= MIN_MARGIN, (c["name"], mf64)
    print(f"{c['name']:24s} valid: delay {delay:7d} k {st['k']:6d} margin {m64:.2e}   "
          f"full: delay {delay_f:7d} k {sf['k']:6d} nb {sf['nb']:6d} margin {mf64:.2e}")
    return dict(delay=np.array(delay, np.int64), k=np.array(st["k"], np.int64),
                margin64=np.array(m64), delay_full=np.array(delay_f, np.int64),
                k_full=np.array(sf["k"], np.int64), nb=np.array(sf["nb"], np.int64),
                margin64_full=np.array(mf64), in_sha=np.array([sha(xt), sha(xb)]),
                meta=np.array(json.dumps(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    a = ap.parse_args()
    sys.path.insert(1, a.ref)
    l2 = importlib.import_module("layer2_analyze_eq")
    ca = importlib.import_module("compare_audio")
    for c in RATIONAL_CASES:
        np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **case(l2, ca, c))


if __name__ == "__main__":
    main()
