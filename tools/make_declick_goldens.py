#!/usr/bin/env python3
"""Generate ``tests/golden/declick_*.npz`` by running the REFERENCE script
``src/declick_inpaint.py`` itself on the cases of ``tests/golden/declick_cases.py``.

Build-container only, like ``tools/make_goldens.py``: the reference imports
``soundfile``, which ``tools/_sf_stub`` stands in for (``sf.read`` serves the
input array, ``sf.write`` captures the float output before PCM quantisation).
Nothing of the reference is copied: a fixture holds the SHA-256 of the float
output, the kept segments, the counts, sigma and thr as float64 bits, the
script's stdout (paths replaced by ``{out}`` / ``{report}``) and its report CSV.

Usage:  python tools/make_declick_goldens.py [--ref /path/to/reference/src]
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import importlib
import io
import json
import os
import re
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests.declick_ref import build_input, sha  # noqa: E402
from tests.golden.declick_cases import CASES  # noqa: E402


def run_case(mod, c, tmp):
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.WRITES.clear()
    x = build_input(c)
    inp, out = os.path.join(tmp, "in.flac"), os.path.join(tmp, "out.flac")
    rep = os.path.join(tmp, "report.csv")
    if os.path.exists(rep):
        os.remove(rep)
    sfstub.STORE[inp] = (x, c["sr"])
    argv = ["declick_inpaint.py", "-i", inp, "-o", out, "--report_csv", rep]
    for k, v in c["params"].items():
        argv += [f"--{k}", str(v)]
    buf = io.StringIO()
    old = sys.argv
    sys.argv = argv
    try:
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the median of nothing (N = 1)
            mod.main()
            # the scalars the script prints with six digits, in full: its own
            # mad_sigma on the statistic it forms (:64-68)
            d = (np.max(np.abs(np.diff(x, axis=0)), axis=1) if len(x) > 1
                 else np.zeros(0, np.float32))
            sigma = mod.mad_sigma(d)
    finally:
        sys.argv = old
    thr = float(c["params"].get("k", 12.0)) * sigma
    text = buf.getvalue()
    y = np.asarray(sfstub.WRITES[out][0])
    hits = int(re.search(r"hits=(\d+)", text).group(1))
    m = re.search(r"\[SEGS\] raw=(\d+), kept=(\d+)", text)
    raw, kept = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    csv_text, segs = "", np.zeros((0, 2), np.int64)
    if os.path.exists(rep):
        with open(rep, newline="", encoding="utf-8") as f:
            csv_text = f.read()
        rows = list(csv.reader(io.StringIO(csv_text, newline="")))[1:]
        segs = np.array([[int(r[0]), int(r[1])] for r in rows], np.int64).reshape(-1, 2)
    assert len(segs) == kept
    assert y.dtype == np.float32 and y.shape == x.shape
    return dict(
        out_sha=np.array(sha(y)), in_sha=np.array(sha(x)), segs=segs,
        raw=np.array(raw, np.int64), hits=np.array(hits, np.int64),
        sigma_bits=np.array(np.float64(sigma).view(np.uint64)),
        thr_bits=np.array(np.float64(thr).view(np.uint64)),
        stdout=np.array(text.replace(rep, "{report}").replace(out, "{out}")),
        report_csv=np.array(csv_text), meta=np.array(json.dumps(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/src")
    a = ap.parse_args()
    sys.path.insert(1, a.ref)
    mod = importlib.import_module("declick_inpaint")
    os.makedirs(OUT_DIR, exist_ok=True)
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            results[c["name"]] = r = run_case(mod, c, tmp)
            print(f"{c['name']:20s} N={c['N']:7d} hits={int(r['hits']):6d} raw={int(r['raw']):4d}"
                  f" kept={len(r['segs']):4d}")
    # conditions on the set
    st = [(c["N"], int(r["hits"]), int(r["raw"]), len(r["segs"]))
          for c, r in ((c, results[c["name"]]) for c in CASES)]
    assert any(k >= 4 and raw - k >= 1 for _, _, raw, k in st), "kept >= 4 and dropped >= 1"
    assert any(k == 0 and h > 0 for _, h, _, k in st), "kept = 0 with hits > 0"
    assert any(h == 0 for _, h, _, _ in st), "hits = 0"
    assert any((n - 1) % 2 == 0 and n > 1 for n, *_ in st), "N - 1 even"
    assert any((n - 1) % 2 == 1 for n, *_ in st), "N - 1 odd"
    for name, r in results.items():
        np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), **r)


if __name__ == "__main__":
    main()
