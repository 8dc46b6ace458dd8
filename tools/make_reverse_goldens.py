#!/usr/bin/env python3
"""Generate ``tests/golden/reverse_*.npz`` by running the REFERENCE tools
``src/reverse_engineer_params.py`` (``analyze_device_params``) and
``src/verify_tilt_amplitude.py`` (``analyze_tilt_detail``) themselves on the
cases of ``tests/golden/reverse_cases.py``.

Build-container only, like ``tools/make_verify_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for.  Nothing of the
reference is copied and a fixture holds no audio: the case, the SHA-256 of the
regenerated x, a decimated sample of y, both scripts' stdout, the CSV's text,
the delay and the float64 margin of the correlation's top behind it, the frame
counts per level bin, the C1 / C2 counts of both scripts
and the histogram counts.

tests/reverse_ref.py's float32 restatement is first checked to reproduce the
reference's CSV, stdout and counts.  Every integer of the output is a decision on
a tilt (the levels are bit-exact on the device and need no margin), so no
frame's float64 tilt may lie within 10 * TI_ATOL of -5, +5 or a histogram edge,
and no level bin's mean tilt that close to 0 (the C1 / C2 word is its sign).

Usage:  python tools/make_reverse_goldens.py --ref /path/to/reference/src
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
from tests import reverse_ref as rr  # noqa: E402
from tests.golden import reverse_cases as rc  # noqa: E402
from tests.golden_util import sha  # noqa: E402

TI_ATOL = 1e-3   # tilt-index means, dB (the project's)
MIN_MARGIN = 1e-3  # the float64 correlation's top over its runner-up (tests/test_align_ref.py)
IN_FILE, OUT_FILE = "in.flac", "out.flac"
SPLIT = "\n正在计算对齐延迟...\n"   # reverse_ref.reverse_text starts here


def captured(fn, *a):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a)
    return out, buf.getvalue()


def check_margins(name, levels, t64):
    edges = sorted({-5, 5} | {e for b in rr.HIST_BINS for e in b})
    dist = np.min(np.abs(t64[:, None] - np.array(edges, np.float64)[None, :]))
    assert dist >= 10 * TI_ATOL, (name, "a tilt on an edge", dist)
    means = [abs(float(np.mean(t64[(lo <= levels) & (levels < hi)])))
             for lo, hi in rr.LEVEL_BINS if np.any((lo <= levels) & (levels < hi))]
    assert min(means) >= 10 * TI_ATOL, (name, "a level bin's mean tilt at 0", min(means))
    return dist, min(means)


def one_case(rev, amp, c, tmp):
    x, y = rc.make_pair(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE[IN_FILE], sfstub.STORE[OUT_FILE] = (x, rc.SR), (y, rc.SR)
    delays = []
    inner = rev.find_delay_xcorr
    rev.find_delay_xcorr = lambda *a, **k: (delays.append(inner(*a, **k)), delays[-1])[1]
    csv_path = os.path.join(tmp, "frames.csv")
    try:
        frame_data, rev_out = captured(rev.analyze_device_params, IN_FILE, OUT_FILE, csv_path)
    finally:
        rev.find_delay_xcorr = inner
    _, amp_out = captured(amp.analyze_tilt_detail, IN_FILE, OUT_FILE)
    with open(csv_path, encoding="utf-8", newline="") as f:
        csv_text = f.read()
    delay = delays[0]
    levels = np.array([f["inp_level"] for f in frame_data], np.float32)
    tilt = np.array([f["tilt"] for f in frame_data], np.float32)

    # the float32 restatement reproduces the reference
    assert rr.find_delay(x, y) == delay, c["name"]
    # the delay is an integer only if the correlation's top stands clear in float64
    m64 = compare_ref.margin(compare_ref.delay_estimate(x, y, rc.SR, 2000, np.float64)["corr"])
    assert m64 >= MIN_MARGIN, (c["name"], m64)
    T = rr.reverse_table(x, y, delay)
    assert np.array_equal(T["levels"], levels), c["name"]
    assert rr.reverse_csv(T["levels"], T["tilts"]) == csv_text, c["name"]
    assert rev_out.endswith(f"\n详细数据已保存: {csv_path}\n")
    body = SPLIT + rev_out.split(SPLIT, 1)[1].rsplit("\n详细数据已保存", 1)[0]
    assert rr.reverse_text(delay, T["n"], T["levels"], T["tilts"]) == body, c["name"]
    counts = rr.reverse_counts(levels, tilt)
    assert counts == rr.reverse_counts(T["levels"], T["tilts"]), c["name"]
    A = rr.amplitude(x, y, delay)
    banner, amp_body = amp_out.split("Delay:", 1)
    assert rr.amplitude_text(A) == "Delay:" + amp_body, (c["name"], rr.amplitude_text(A), amp_out)

    # no decision on an edge
    t64 = rr.reverse_table(x, y, delay, dtype=np.float64)["tilts"]
    dist, m0 = check_margins(c["name"], levels, t64)
    assert counts == rr.reverse_counts(levels, t64), c["name"]
    print(f"{c['name']:20s} delay {delay:6d} F {len(levels):4d} bins {counts['level_bins']} "
          f"C1/C2 {counts['c1']}/{counts['c2']} amp {A['n_c1']}/{A['n_c2']} "
          f"edge margin {dist:.3f} dB, mean-tilt margin {m0:.3f} dB, xcorr margin {m64:.1e}")

    return dict(meta=np.array(json.dumps(c)), x_sha=np.array(sha(x)),
                y_dec=np.ascontiguousarray(y[::rc.DECIM]), y_len=np.array(len(y), np.int64),
                delay=np.array(delay, np.int64), margin64=np.array(m64), n_aligned=np.array(T["n"], np.int64),
                reverse_stdout=np.array(body), csv=np.array(csv_text),
                level_bins=np.array(counts["level_bins"], np.int64),
                tilt_classes=np.array([counts["c1"], counts["c2"]], np.int64),
                hist=np.array(counts["hist"], np.int64),
                amp_stdout=np.array(banner + "Delay:" + amp_body),
                amp_classes=np.array([A["n_c1"], A["n_c2"]], np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    ap.add_argument("--only", default=None, help="one case name")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    rev = importlib.import_module("reverse_engineer_params")
    amp = importlib.import_module("verify_tilt_amplitude")
    for c in rc.CASES:
        if a.only and c["name"] != a.only:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"),
                                **one_case(rev, amp, c, tmp))


if __name__ == "__main__":
    main()
