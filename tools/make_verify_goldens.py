#!/usr/bin/env python3
"""Generate ``tests/golden/verify_*.npz`` by running the REFERENCE validators
``src/verify_tomatis_15db_v2.py`` and ``src/validate_layer1.py`` themselves
(their ``main``) on the cases of ``tests/golden/verify_cases.py``.

Build-container only, like ``tools/make_baseline_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for, and matplotlib,
which runs with ``MPLBACKEND=Agg``.  Nothing of the reference is copied and a
fixture holds no audio: the case, the SHA-256 of the regenerated x, a decimated
sample of y, stdout, the report text, the exit code, the CSV's four value
columns as float32, the frame counts, the solved threshold and its C2 share, the
switch count, the SHA-256 of the state string, the peak's bits, the DC mean, the
tilt-index statistics, and each criterion's value, threshold and device
tolerance.  tests/verify_ref.py's restatement is first checked to reproduce the
reference's CSV columns, counts and report; every PASS / FAIL / WARN word must
sit at least ten device tolerances from its threshold.

Usage:  python tools/make_verify_goldens.py --ref /path/to/reference/src
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
from tests import verify_ref as vr  # noqa: E402
from tests.golden import verify_cases as vc  # noqa: E402
from tests.golden_util import sha  # noqa: E402

DB_ATOL = 2e-3   # conditional spectra, dB (tests/test_gpu_analysis.py)
TI_ATOL = 1e-3   # tilt-index means, dB
DC_RTOL = 2.0 ** -20
CSV_HEADER = "freq_hz,c1_measured_db,c1_theory_db,c2_measured_db,c2_theory_db"
IN_FILE, OUT_FILE = "in.flac", "out.flac"


def flags(a, skip=()):
    out = []
    for k, v in a.items():
        if k not in skip:
            out += ["--" + k, str(v)]
    return out


def record(mod, names):
    """Wrap mod.<name> so that every return value is kept: -> (log, restore)."""
    log = {n: [] for n in names}
    inner = {n: getattr(mod, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            log[n].append(inner[n](*a, **k))
            return log[n][-1]
        return f

    for n in names:
        setattr(mod, n, wrap(n))

    def restore():
        for n in names:
            setattr(mod, n, inner[n])
    return log, restore


def run_main(mod, argv, tmp, names):
    buf = io.StringIO()
    cwd, old = os.getcwd(), sys.argv
    os.chdir(tmp)
    log, restore = record(mod, names)
    sys.argv = ["prog"] + argv
    try:
        with contextlib.redirect_stdout(buf):
            rc = mod.main()
    finally:
        restore()
        sys.argv = old
        os.chdir(cwd)
    return rc, buf.getvalue(), log


def read_csv(path):
    with open(path, encoding="utf-8") as f:
        header = f.readline().strip()
    assert header == CSV_HEADER, header
    return np.loadtxt(path, delimiter=",", skiprows=1)


def codes_of(states):
    return np.array([1 if s == "C1" else 2 for s in states], np.int8)


def check_margins(name, margins, words):
    for k, (v, thr, tol) in margins.items():
        d = abs(v - thr)
        assert d >= 10 * tol and d > 0, (name, k, v, thr, tol)
    print(f"{name:24s} {words}  min margin/tol "
          f"{min((abs(v - t) / tol for v, t, tol in margins.values() if tol > 0), default=np.inf):.1f}")


def common(c, x, y):
    return dict(meta=np.array(json.dumps(c)), x_sha=np.array(sha(x)),
                y_dec=np.ascontiguousarray(y[::vc.DECIM]), y_len=np.array(len(y), np.int64))


def v2_case(mod, c, tmp):
    x, y, _ = vc.make_pair(c)
    a = vc.v2_args(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE[IN_FILE], sfstub.STORE[OUT_FILE] = (x, vc.SR), (y, vc.SR)
    rc, text, log = run_main(
        mod, ["-i", IN_FILE, "-o", OUT_FILE] + flags(a), tmp,
        ["check_engineering", "find_optimal_threshold", "simulate_gate_with_threshold",
         "find_stable_frames", "compute_conditional_spectrum_v2", "compute_tilt_index",
         "compute_frame_levels"])
    prefix = os.path.join(tmp, a["out_prefix"])
    cols = read_csv(prefix + "_spectrum.csv")
    with open(prefix + "_report.txt", encoding="utf-8") as f:
        report = f.read()
    for suffix in ("_spectrum.png", "_tilt_index.png"):
        assert os.path.getsize(prefix + suffix) > 0
    eng = log["check_engineering"][0]
    T, ratio = log["find_optimal_threshold"][0]
    codes = codes_of(log["simulate_gate_with_threshold"][-1])
    levels = np.asarray(log["compute_frame_levels"][0])
    s1, s2 = log["find_stable_frames"][0]
    _, _, _, n1, n2 = log["compute_conditional_spectrum_v2"][0]
    ti = log["compute_tilt_index"][0]

    # the restatement reproduces the reference
    R = vr.run_v2(x, y, vc.SR, a)
    assert np.array_equal(R["levels"], levels), c["name"]
    assert (R["T"], R["ratio"]) == (T, ratio) and np.array_equal(R["codes"], codes), c["name"]
    assert (R["c1_n"], R["c2_n"]) == (n1, n2), c["name"]
    assert [len(v) for v in vr.stable(codes)] == [len(s1), len(s2)]
    assert np.array_equal(vr.csv_columns(R), cols[:, 1:]), c["name"]
    assert vr.report_v2(R) == report, (c["name"], vr.report_v2(R), report)
    assert R["peak"] == eng["peak"] and int(not R["ok"]) == rc
    keys = ("input", "output", "c1", "c2")
    for k in keys:
        assert len(R["ti_data"][k]) == len(ti[k]), (c["name"], k)
        assert np.allclose(R["ti_data"][k], ti[k], rtol=0, atol=1e-4), (c["name"], k)

    m = R["metrics"]
    margins = {"peak": (float(eng["peak"]), 0.98, 0.0),
               "dc": (abs(R["dc"]), 0.001, DC_RTOL * abs(R["dc"])),
               "c2_lo": (R["c2_ratio"], 0.48, 0.0), "c2_hi": (R["c2_ratio"], 0.52, 0.0)}
    for k in ("c1_lo_platform_rmse", "c2_lo_platform_rmse", "c1_hi_platform_rmse",
              "c2_hi_platform_rmse", "c1_fc_error", "c2_fc_error"):
        margins[k] = (float(m.get(k, 99)), 0.5, DB_ATOL)
    for k in ("c1_slope_rmse", "c2_slope_rmse"):
        margins[k] = (float(m.get(k, 99)), 1.0, DB_ATOL)
    margins["ti_effect"] = (float(R["ti_effect"]), 20.0, 2 * TI_ATOL)
    check_margins(c["name"], margins, f"exit {rc} T {T:.2f} C2 {ratio*100:.1f}% used {n1}/{n2} "
                  f"ti {float(R['ti_effect']):.1f}")

    def stat(fn):
        return np.array([fn(ti[k]) if len(ti[k]) else np.nan for k in keys], np.float64)

    d = common(c, x, y)
    d.update(stdout=np.array(text), report=np.array(report), exit_code=np.array(rc, np.int64),
             cols=cols[:, 1:].astype(np.float32), freq_col=cols[:, 0],
             stable=np.array([len(s1), len(s2)], np.int64), used=np.array([n1, n2], np.int64),
             T=np.array(float(T)), ratio=np.array(float(ratio)),
             switch_count=np.array(vr.switches(codes), np.int64),
             n_levels=np.array(len(levels), np.int64), state_sha=np.array(vr.state_sha(codes)),
             levels_sha=np.array(sha(levels)),
             peak_bits=np.array(np.float32(eng["peak"]).view(np.uint32)),
             dc=np.array(R["dc"]), dc_ref32=np.array(float(eng["dc_mean"])),
             ti_mean=stat(np.mean), ti_std=stat(np.std),
             ti_n=np.array([len(ti[k]) for k in keys], np.int64),
             margin_keys=np.array(json.dumps(list(margins))),
             margins=np.array([margins[k] for k in margins], np.float64))
    return d


def l1_case(mod, c, tmp):
    x, y, rows = vc.make_pair(c)
    a = vc.l1_args(c)
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.STORE[IN_FILE], sfstub.STORE[OUT_FILE] = (x, vc.SR), (y, vc.SR)
    csv_path = os.path.join(tmp, "state.csv")
    vc.write_state_csv(csv_path, rows)
    rc, text, log = run_main(
        mod, ["-i", IN_FILE, "-o", OUT_FILE, "--state_csv", csv_path] + flags(a), tmp,
        ["check_engineering", "simulate_gate", "compare_gate_states",
         "compute_conditional_spectrum"])
    cols = read_csv(os.path.join(tmp, a["out_csv"]))
    assert os.path.getsize(os.path.join(tmp, a["out_png"])) > 0
    eng = log["check_engineering"][0]
    sim_states, sim_levels = log["simulate_gate"][0]
    cmp = log["compare_gate_states"][0]
    _, _, _, n1, n2 = log["compute_conditional_spectrum"][0]

    R = vr.run_l1(x, y, vc.SR, rows, a)
    assert np.array_equal(R["levels"], np.asarray(sim_levels)), c["name"]
    assert np.array_equal(R["sim"], codes_of(sim_states)), c["name"]
    assert (R["mismatch"], R["csv_switches"], R["sim_switches"], R["total"]) == \
        (cmp["mismatch_count"], cmp["csv_switches"], cmp["sim_switches"], cmp["total_frames"])
    assert R["level_max_diff"] == cmp["level_max_diff"]
    assert (R["c1_n"], R["c2_n"]) == (n1, n2), c["name"]
    assert np.array_equal(vr.csv_columns(R), cols[:, 1:]), c["name"]
    assert R["peak"] == eng["peak"] and int(not R["ok"]) == rc

    margins = {"peak": (float(eng["peak"]), 0.98, 0.0),
               "mismatch_rate": (R["mismatch_rate"], 0.01, 0.0),
               "level_max_diff": (R["level_max_diff"], 0.1, 0.0),
               "rmse_max": (float(max(R["rmse"])), 1.5, DB_ATOL)}
    check_margins(c["name"], margins, f"exit {rc} mismatch {R['mismatch']} used {n1}/{n2} "
                  f"rmse max {float(max(R['rmse'])):.3f}")
    d = common(c, x, y)
    d.update(stdout=np.array(text), exit_code=np.array(rc, np.int64),
             cols=cols[:, 1:].astype(np.float32), freq_col=cols[:, 0],
             used=np.array([n1, n2], np.int64), mismatch=np.array(R["mismatch"], np.int64),
             total=np.array(R["total"], np.int64),
             csv_switches=np.array(R["csv_switches"], np.int64),
             sim_switches=np.array(R["sim_switches"], np.int64),
             level_max_diff=np.array(R["level_max_diff"]),
             state_sha=np.array(vr.state_sha(R["sim"])), levels_sha=np.array(sha(R["levels"])),
             peak_bits=np.array(np.float32(eng["peak"]).view(np.uint32)),
             rmse=np.array(R["rmse"], np.float64),
             margin_keys=np.array(json.dumps(list(margins))),
             margins=np.array([margins[k] for k in margins], np.float64))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's src directory")
    ap.add_argument("--only", default=None, help="one case name")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    v2 = importlib.import_module("verify_tomatis_15db_v2")
    l1 = importlib.import_module("validate_layer1")
    for cases, mod, fn in ((vc.V2_CASES, v2, v2_case), (vc.L1_CASES, l1, l1_case)):
        for c in cases:
            if a.only and c["name"] != a.only:
                continue
            with tempfile.TemporaryDirectory() as tmp:
                np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **fn(mod, c, tmp))


if __name__ == "__main__":
    main()
