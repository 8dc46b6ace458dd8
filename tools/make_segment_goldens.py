#!/usr/bin/env python3
"""Generate ``tests/golden/seg_*.npz`` and ``cut_*.npz`` by running the REFERENCE
scripts themselves, ``src/find_main_segment.py`` (its ``main()``) and
``src/cut_tomatis_d.py`` (its ``cut_audio``), on the cases of
``tests/golden/segment_cases.py``.

Build-container only, like ``tools/make_declick_goldens.py``: the reference
imports ``soundfile``, which ``tools/_sf_stub`` stands in for
(``SoundFile.read`` / ``sf.read`` serve the input array, ``sf.write`` captures
the float output before PCM quantisation).  Nothing of the reference is copied.
A segment fixture holds the script's stdout, the levels its own
``win_rms_dbfs`` returns for every window as float32 bits, ``noise_floor`` and
``thr`` as float64 bits, and the type and text of the exception where it raised;
a cut fixture the stdout (paths replaced by ``{in}`` / ``{out}``) and the
SHA-256 and length of the array the script wrote.

Usage:  python tools/make_segment_goldens.py [--ref /path/to/reference/src]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT_DIR = os.path.join(REPO, "tests", "golden")

sys.path.insert(0, os.path.join(HERE, "_sf_stub"))
sys.path.insert(0, REPO)
import soundfile as sfstub  # noqa: E402  (the stand-in)
from tests import segment_ref as sr_  # noqa: E402
from tests.golden.segment_cases import CUT_CASES, SEGMENT_CASES  # noqa: E402


def _reset():
    sfstub.GUARD_BYPASS = False
    sfstub.STORE.clear()
    sfstub.WRITES.clear()


def run_segment(mod, c):
    _reset()
    x = sr_.build_input(c["name"])
    sfstub.STORE["in.flac"] = (x, c["sr"])
    p = c["params"]
    buf = io.StringIO()
    old, exc = sys.argv, ("", "")
    sys.argv = ["find_main_segment.py", "-i", "in.flac"] + sr_.cli_args(p)
    try:
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                mod.main()
            except Exception as e:  # recorded: the device module raises the same
                exc = (type(e).__name__, str(e))
    finally:
        sys.argv = old
    # the levels of every window through the script's own win_rms_dbfs, and its
    # own scalar expressions for the two numbers it prints with one digit
    sr = c["sr"]
    win = int(sr * p.get("win_ms", 100.0) / 1000.0)
    hop = int(sr * p.get("hop_ms", 50.0) / 1000.0)
    lv = []
    if x.shape[1] == 2:
        s = 0
        while s + win <= len(x):
            lv.append(mod.win_rms_dbfs(x[s:s + win]))
            s += hop
    lv = np.array(lv, np.float32)
    nf = thr = float("nan")
    if len(lv):
        nf = float(np.percentile(lv, 10))
        thr = nf + p.get("margin_db", 15.0)
    return dict(stdout=np.array(buf.getvalue()), levels_bits=lv.view(np.uint32),
                noise_floor_bits=np.array(np.float64(nf).view(np.uint64)),
                thr_bits=np.array(np.float64(thr).view(np.uint64)),
                exc_type=np.array(exc[0]), exc_text=np.array(exc[1]),
                in_sha=np.array(sr_.sha(x)), meta=np.array(json.dumps(c)))


def run_cut(mod, c):
    _reset()
    x = sr_.build_input(c["name"])
    sfstub.STORE["in.flac"] = (x, c["sr"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if c["cut_seconds"] is None:
            mod.cut_audio("in.flac", "out.flac")
        else:
            mod.cut_audio("in.flac", "out.flac", c["cut_seconds"])
    y = np.asarray(sfstub.WRITES["out.flac"][0])
    assert y.dtype == np.float32 and sfstub.WRITES["out.flac#sr"] == c["sr"]
    text = buf.getvalue().replace("in.flac", "{in}").replace("out.flac", "{out}")
    return dict(stdout=np.array(text), out_sha=np.array(sr_.sha(y)),
                out_len=np.array(len(y), np.int64), in_sha=np.array(sr_.sha(x)),
                meta=np.array(json.dumps(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/src")
    a = ap.parse_args()
    sys.path.insert(1, a.ref)
    fms = importlib.import_module("find_main_segment")
    cut = importlib.import_module("cut_tomatis_d")
    os.makedirs(OUT_DIR, exist_ok=True)
    res = {}
    for c in SEGMENT_CASES:
        res[c["name"]] = r = run_segment(fms, c)
        print(f"{c['name']:20s} F={len(r['levels_bits']):5d} exc={str(r['exc_type'])!r:14s} "
              f"{str(r['stdout']).splitlines()[-1] if str(r['stdout']) else ''}")
    for c in CUT_CASES:
        res[c["name"]] = r = run_cut(cut, c)
        print(f"{c['name']:20s} wrote {int(r['out_len'])} frames")
    # conditions on the set
    out = {k: str(v["stdout"]) for k, v in res.items()}
    two = next(c for c in SEGMENT_CASES if c["name"] == "seg_96k_two_equal")
    lv, tm, win_sec = sr_.levels(sr_.build_input(two["name"]), two["sr"], two["params"]["win_ms"],
                                 two["params"]["hop_ms"])
    thr = float(np.float64(res[two["name"]]["thr_bits"].view(np.float64)))
    lens = [float(tm[j - 1] + win_sec) - float(tm[i]) for i, j in sr_.runs(lv >= thr)]
    assert len(lens) == 2 and lens[0] == lens[1], lens
    assert "start=1.438s" in out["seg_96k_two_equal"].splitlines()[4], "the first of two equal"
    assert "start=0.000s" in out["seg_44k_pad0"].splitlines()[5], "the pad clamps at 0"
    assert "end=6.000s" in out["seg_44k_odd_end"].splitlines()[5], "the pad clamps at dur"
    assert out["seg_48k_one"].count("\n") == 6
    assert out["seg_48k_none"].startswith("未找到") and out["seg_44k_short"].startswith("最长段")
    assert str(res["seg_48k_tiny"]["exc_type"]) and str(res["seg_48k_mono"]["exc_type"]) == \
        "ValueError"
    for name, r in res.items():
        np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), **r)


if __name__ == "__main__":
    main()
