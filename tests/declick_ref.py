"""Test-local numpy statement of the de-click stage (what
tomatis_audio_processor_amd/declick_inpaint.py computes on the device), written
from the rules and not from the reference's code, plus the builder of the golden
cases' inputs.  The CPU tests hold it against the goldens the reference
produced; the GPU tests hold the device against it."""
from __future__ import annotations

import hashlib
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tomatis_audio_processor_amd.synth import synth_stream  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden(name: str) -> dict:
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def quantise(x: np.ndarray, bits: int):
    """(integer PCM, the float32 samples a file of that PCM decodes to)."""
    full = float(1 << (bits - 1))
    q = np.clip(np.rint(np.asarray(x, np.float64) * full), -(full - 1), full - 1)
    return q.astype(np.int32), (q / full).astype(F32)


def noise_clicks(seed, n, ch, sr, bits, clicks=(), n_random=0, bursts=()):
    """Sine + stationary noise with additive clicks and bursts, quantised."""
    # synth_stream's envelope switches level every 1.5 "seconds": a huge nominal
    # rate and an offset past the first ramp keep it on its quiet level
    noise = synth_stream(seed, n, ch, 10_000_000, start=1_000_000).astype(np.float64) * 10.0
    t = np.arange(n, dtype=np.float64) / sr
    x = noise + 0.2 * np.sin(2.0 * np.pi * 440.0 * t[:, None] + 0.5 * np.arange(ch)[None, :])
    rng = np.random.default_rng(seed)
    pos = [int(p) for p in clicks]
    if n_random:
        pos += [int(p) for p in np.sort(rng.choice(n, size=n_random, replace=False))]
    for p in pos:
        amp = rng.uniform(0.3, 0.6) * (1.0 if rng.integers(2) else -1.0)
        c = int(rng.integers(ch + 1))
        if c == ch:
            x[p, :] += amp      # a click on every channel
        else:
            x[p, c] += amp
    for s, ln in bursts:
        x[s:s + ln] += rng.uniform(-0.5, 0.5, size=(ln, ch))
    return quantise(np.clip(x, -0.999, 0.999), bits)


def build_input_pcm(c: dict):
    n, ch, bits = c["N"], c["ch"], c["bits"]
    if c["kind"] == "zero":
        return quantise(np.zeros((n, ch)), bits)
    if c["kind"] == "square":
        sq = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        return quantise(np.repeat(sq[:, None], ch, axis=1), bits)
    return noise_clicks(c["seed"], n, ch, c["sr"], bits, c["clicks"], c["n_random"], c["bursts"])


def build_input(c: dict) -> np.ndarray:
    return build_input_pcm(c)[1]


# ---------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------
def detection_statistic(x: np.ndarray) -> np.ndarray:
    """Largest absolute sample-to-sample step over the channels, float32 [N-1]."""
    x = np.asarray(x, F32)
    if len(x) < 2:
        return np.zeros(0, F32)
    return np.abs(x[1:] - x[:-1]).max(axis=1)


def robust_sigma(d: np.ndarray) -> float:
    """MAD scale in float32: (median |d - median d| + 1e-12) / 0.6745."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        centre = np.median(d)
        spread = np.median(np.abs(d - centre)) + 1e-12
    return float(spread / 0.6745)


def clusters(hit_idx: np.ndarray, n: int, pad: int, gap: int) -> np.ndarray:
    """Closed form of pad -> mask -> merge: hits no further apart than
    2 pad + 1 + gap share a segment [first - pad, last + 1 + pad), clipped."""
    if hit_idx.size == 0:
        return np.zeros((0, 2), np.int64)
    far = np.flatnonzero(np.diff(hit_idx) > 2 * pad + 1 + gap)
    a = hit_idx[np.concatenate(([0], far + 1))]
    b = hit_idx[np.concatenate((far, [hit_idx.size - 1]))]
    return np.stack([np.maximum(0, a - pad), np.minimum(n, b + 1 + pad)], axis=1).astype(np.int64)


def inpaint(x: np.ndarray, segs: np.ndarray) -> np.ndarray:
    """Each segment [s, e) becomes the float32 line between its neighbours
    x[s-1] and x[e] (clipped to the file), weights from a double-precision ramp."""
    y = x.copy()
    n = len(x)
    one = F32(1)
    for s, e in segs:
        s0, e0 = max(0, int(s) - 1), min(n - 1, int(e))
        if s0 >= e0:
            continue
        span = e0 - s0
        i = np.arange(int(s) - s0, int(e) - s0)
        t = (i.astype(np.float64) * (1.0 / span)).astype(F32)
        t[i == span] = one
        y[s:e] = (one - t)[:, None] * x[s0][None, :] + t[:, None] * x[e0][None, :]
    return y


def declick(x, sr, k=12.0, pad_ms=1.5, merge_gap_ms=0.5, max_fix_ms=8.0) -> dict:
    x = np.asarray(x, F32)
    n = len(x)
    d = detection_statistic(x)
    sigma = robust_sigma(d)
    thr = k * sigma
    with np.errstate(invalid="ignore"):
        hit_idx = np.flatnonzero(d > F32(thr))
    none = np.zeros((0, 2), np.int64)
    if hit_idx.size == 0:
        return dict(y=x.copy(), segs=none, raw=0, hits=0, sigma=sigma, thr=thr)
    pad = int(round(pad_ms * sr / 1000.0))
    gap = int(round(merge_gap_ms * sr / 1000.0))
    max_fix = int(round(max_fix_ms * sr / 1000.0))
    raw = clusters(hit_idx, n, pad, gap)
    segs = raw[(raw[:, 1] - raw[:, 0]) <= max_fix]
    return dict(y=inpaint(x, segs), segs=segs, raw=len(raw), hits=int(hit_idx.size),
                sigma=sigma, thr=thr)


def pcm24_of(y: np.ndarray) -> np.ndarray:
    """The PCM_24 samples a float file write stores (libsndfile's rule)."""
    return np.clip(np.rint(np.asarray(y, np.float64) * 8388607.0), -8388608, 8388607).astype(
        np.int32)


def report_text(segs: np.ndarray, sr: int) -> str:
    """The report CSV of the kept segments (csv.writer, Python float text)."""
    import csv
    import io
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["start_sample", "end_sample", "start_sec", "end_sec", "len_samples"])
    for s, e in segs:
        w.writerow([int(s), int(e), s / sr, e / sr, int(e - s)])
    return buf.getvalue()


def f64_bits(v: float) -> int:
    return int(np.float64(v).view(np.uint64))
