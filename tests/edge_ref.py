"""The error model of conditioning.py as a per-sample bound, and the cases on
which the device is held to it (tests/test_edge_ref.py on the CPU,
tests/test_gpu_edge_samples.py on the device).

Every other sample-level test masks the output samples whose window sum
``sum w^2`` is below ``TAU``: the heads and tails of streams.  Here nothing is
masked.  For one stream

    |y(p) - y64(p)| <= D(p) = KAPPA_INT * A(p) + KAPPA_EDGE * A(p) * S1(p) / den(S2(p))

for every output sample p of every channel, with y64 the float64 statement of
the operation (``stft_ref.stft_ref``), S1 / S2 the sums of w and w^2 of the
frames covering p (``conditioning.window_sums``), ``den`` the processor's
normaliser (``conditioning._den``) and A(p) the largest well-conditioned
|y64| (S2 >= TAU, any channel) within +-n_fft of p.  This is the term
``conditioning.chunk_flags`` builds, for one implementation (no factor 2 for a
pair).  Where D(p) == 0 no well-conditioned energy lies within a frame of p
and the output must be an exact zero.

Cases: streams of 5 to 9 frames, one per tail class of the framing
(``lengths``), white noise in a loud and a quiet block so that both gate
states occur, independent random gains per bin and row.  The per-frame rows of
the gate pipelines come from the oracle's gate here and from the pipeline on
the device (asserted equal there).
"""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np

from oracle import tomatis_oracle as orc
from tests.stft_ref import case_rows, static_geometry, stft_ref, white
from tomatis_audio_processor_amd import conditioning as cd
from tomatis_audio_processor_amd import dsp

SR = 48000
F_MIN, F_MAX = 5, 9

# the shapes conditioning.py's constants were calibrated on
CORE = [(2048, 512), (2048, 256), (4096, 1024), (4096, 2048), (2048, 300)]
# beyond them: any-size path in LDS (Stockham, Bluestein), per-block HBM buffers
EXTENDED = [(1024, 256), (512, 128), (3000, 750), (100, 25), (12000, 3000)]

# standard mode runs with an output gain of 2^-24 (exact in float32: the
# reference is scaled by the same power of two), which keeps 1 / sum w^2 times
# the filter's time-aliased tail under the limiter
STD_GAIN_LOG2 = -24

TAILS = ("tail0", "mid", "plus1")


# ---------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------

def local_amplitude(y64, s2, n_fft):
    """A(p): the largest |y64| over channels among samples with s2 >= TAU
    within +-n_fft of p (0 where there is none)."""
    ya = np.abs(np.asarray(y64, np.float64).reshape(len(s2), -1)).max(axis=1)
    q = np.arange(len(s2), dtype=np.int64)
    good = np.asarray(s2) >= cd.TAU
    gq, gy = q[good], ya[good]
    if len(gq) == 0:
        return np.zeros(len(s2))
    lo = np.searchsorted(gq, q - n_fft, "left")
    hi = np.searchsorted(gq, q + n_fft, "right")
    return cd._range_max(gy, lo, hi)


def sample_bound(y64, s1, s2, n_fft, norm):
    """D(p) for every output sample (module docstring)."""
    A = local_amplitude(y64, s2, n_fft)
    return cd.KAPPA_INT * A + cd.KAPPA_EDGE * A * np.asarray(s1) / cd._den(np.asarray(s2), norm)


def ratios(y, y64, D, s2):
    """(largest err / D over all samples with D > 0, the same over the samples
    the other tests mask, largest |y| where D == 0)."""
    err = np.abs(np.asarray(y, np.float64) - y64).max(axis=1)
    pos = D > 0
    r = np.zeros(len(D))
    r[pos] = err[pos] / D[pos]
    masked = pos & (np.asarray(s2) < cd.TAU)
    z = np.abs(np.asarray(y, np.float64))[~pos]
    return (float(r.max(initial=0.0)), float(r[masked].max(initial=0.0)),
            float(z.max(initial=0.0)))


# ---------------------------------------------------------------------------
# stream lengths, one per tail class
# ---------------------------------------------------------------------------

def _remainder(tail, hop):
    return {"tail0": 0, "mid": (hop // 2 + 3) % hop, "plus1": 1 % hop}[tail]


def lengths(mode, n_fft, hop):
    """{tail class: N}: the shortest streams of F_MIN + 1 .. F_MAX frames in
    each tail class of ``mode``'s framing, each class one frame longer than the
    one before.

    standard / xfade (orc._std_schedule: front pad n_fft / 2, end pad pe):
      tail0   pe == 0: the last frame ends at N (hop divides n_fft / 2) and
              sum w^2 runs down to 0 at N - 1
      mid     N - n_fft leaves hop // 2 + 3 of a hop (2048 / 512: the 259 of
              the golden std_48k_st_2048_512_tail259)
      plus1   one sample past a frame boundary: pe == hop - 1
    adaptive (dsp.adaptive_frames: frames from 0, sum w^2 == 0 at sample 0) and
    static EQ (stft_ref.static_geometry, pad or not): the same three remainders
    of N - n_fft."""
    out = {}
    for i, tail in enumerate(TAILS):
        want_f = F_MIN + 1 + i
        rem = _remainder(tail, hop)
        for N in range(n_fft, n_fft + (F_MAX + 2) * hop + 1):
            if mode in ("std", "xfade"):
                _, pe, F, _ = orc._std_schedule(N, n_fft, hop)
                ok = pe == (hop - rem) % hop
            elif mode == "adaptive":
                _, F, s0 = dsp.adaptive_frames(N, n_fft, hop)
                ok = (N - n_fft) % hop == rem and s0 == 0
            else:
                F = static_geometry(N, n_fft, hop, mode == "static_pad")["n_frames"]
                ok = (N - n_fft) % hop == rem
            if ok and F == want_f:
                out[tail] = N
                break
        else:
            raise AssertionError((mode, n_fft, hop, tail))
    assert len(set(out.values())) == len(TAILS)
    return out


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

def _c(mode, n_fft, hop, ch, path):
    return [(mode, n_fft, hop, ch, tail, path) for tail in TAILS]


# (mode, n_fft, hop, channels, tail class, kernel path)
GATE_CASES = (
    [c for ch in (1, 2) for c in _c("std", 2048, 512, ch, "gated 2048")]
    + [c for ch in (1, 2) for c in _c("std", 2048, 256, ch, "gated 2048")]
    + [c for ch in (1, 2) for c in _c("std", 4096, 1024, ch, "4096")]
    + [c for ch in (1, 2) for c in _c("std", 2048, 300, ch, "generic hop")]
    + [c for ch in (1, 2) for c in _c("xfade", 4096, 2048, ch, "4096 xfade")])
ADAPTIVE_CASES = (
    [c for ch in (1, 2) for c in _c("adaptive", 2048, 512, ch, "adaptive 2048")]
    + _c("adaptive", 1024, 256, 2, "adaptive LDS pow2")
    + _c("adaptive", 3000, 750, 2, "adaptive LDS Bluestein"))
STATIC_CASES = [c for mode in ("static_pad", "static_nopad") for c in (
    [c for ch in (1, 2) for c in _c(mode, 4096, 2048, ch, "static 4096")]
    + _c(mode, 512, 128, 3, "static LDS pow2")
    + _c(mode, 100, 25, 2, "static LDS Bluestein")
    + _c(mode, 12000, 3000, 1, "static HBM"))]
ALL_CASES = GATE_CASES + ADAPTIVE_CASES + STATIC_CASES


def case_id(case):
    mode, n_fft, hop, ch, tail, _ = case
    return f"{mode}-{n_fft}/{hop}-ch{ch}-{tail}"


def _seed(case):
    mode, n_fft, hop, ch, tail, _ = case
    return (7 * n_fft + 3 * hop + 11 * ch + 1000 * TAILS.index(tail)
            + 100000 * ["std", "xfade", "adaptive", "static_pad", "static_nopad"].index(mode))


def gate_params(n_fft, hop, amp, xfade, gain_log2=STD_GAIN_LOG2):
    """Loud block at amp / sqrt(3) RMS, quiet one 30 dB below, the threshold
    half way; an up-delay of 1.5 frames; cross-fade over 2.5 frames."""
    T = 20.0 * np.log10(amp / np.sqrt(3.0)) - 15.0
    p = dict(gate_ui=T + 100.0, gate_mode="linear", n_fft=n_fft, hop=hop,
             up_delay_ms=1.5 * hop / SR * 1000.0)
    if xfade:
        p["xfade_ms"] = 2.5 * hop / SR * 1000.0
    else:
        p["output_gain_db"] = 20.0 * np.log10(2.0 ** gain_log2)   # float32(10^(dB / 20)) == 2^k
    return p


def adaptive_params(n_fft, hop):
    return dict(n_fft=n_fft, hop=hop, min_hold_ms=1.5 * hop / SR * 1000.0,
                xfade_ms=2.5 * hop / SR * 1000.0)


def xfade_rows(states, alpha, xf):
    """Gain-row ids of a cross-fade plan (tomatis_gate_std): 0 / 1 at the
    snapped ends, 2 + m at alpha = m / xf."""
    a = np.asarray(alpha, np.float64)
    mid = (a > 0.0) & (a < 1.0) if xf > 0 else np.zeros(len(a), bool)
    return np.where(mid, 2 + np.rint(a * xf).astype(np.int64), (a >= 0.5).astype(np.int64))


def signal(case, N, silent_edges=0, amp=None):
    """``stft_ref.white`` in two blocks: a quiet one (1 / 32) over the first two
    frames (streams this short have no room for a whole quiet frame anywhere
    else: the front pad makes the first frames short), the rest loud, so that
    the gate switches and the tail carries the loud block.  ``silent_edges``:
    that many samples of digital silence at both ends."""
    mode, n_fft, hop, ch, tail, _ = case
    if amp is None:
        amp = 0.125 if mode == "adaptive" else 0.5
    body = N - 2 * silent_edges
    first = n_fft // 2 if mode in ("std", "xfade") else n_fft   # end of frame 0 in the stream
    w = white(_seed(case), body, ch, amp=amp)
    w[:min(first + hop, body // 2)] *= np.float32(1.0 / 32)
    x = np.zeros((N, ch), np.float32)
    x[silent_edges:N - silent_edges] = w
    return x


@functools.lru_cache(maxsize=None)
def build(case, silent_edges=0, amp=None, N=None, gain_log2=STD_GAIN_LOG2):
    """One stream of ``case``: input, pipeline parameters, float64 gain table,
    per-frame rows (the oracle's gate), C-ABI geometry, norm rule and output
    scale.  Cached and read-only."""
    mode, n_fft, hop, ch, tail, path = case
    short = N is None and not silent_edges
    if N is None:
        N = lengths(mode, n_fft, hop)[tail] + 2 * silent_edges
    x = signal(case, N, silent_edges, amp)
    bins = n_fft // 2 + 1
    c = SimpleNamespace(case=case, mode=mode, n_fft=n_fft, hop=hop, ch=ch, tail=tail, path=path,
                        N=N, x=x, norm="eps", out_scale=1.0, oref=None, params={}, xf=0)
    if mode in ("std", "xfade"):
        c.params = gate_params(n_fft, hop, 0.5 if amp is None else amp, mode == "xfade", gain_log2)
        c.oref = orc.process_standard(x, SR, **c.params)
        pad, pe, F, starts = orc._std_schedule(N, n_fft, hop)
        c.geom = dict(first_start=-pad, n_frames=F, hop=hop, out_begin=0, out_len=N)
        if mode == "xfade":
            c.xf = int(np.ceil(c.params["xfade_ms"] / (hop / SR * 1000.0)))
            c.rows = xfade_rows(c.oref["states"], c.oref["alpha"], c.xf)
            c.n_rows = 2 + c.xf + 1
        else:
            c.rows = c.oref["states"].astype(np.int64) - 1
            c.n_rows = 2
            c.out_scale = 2.0 ** gain_log2
    elif mode == "adaptive":
        c.params = adaptive_params(n_fft, hop)
        c.oref = orc.process_adaptive(x, SR, **c.params)
        assert c.oref["atten_db"] == 0, "no attenuation: in_scale = out_scale = 1"
        _, F, s0 = dsp.adaptive_frames(N, n_fft, hop)
        c.geom = dict(first_start=s0, n_frames=F, hop=hop, out_begin=0, out_len=N)
        c.xf = int(c.oref["xfade_frames"])
        c.rows = 2 + np.rint(np.asarray(c.oref["alpha"]) * c.xf).astype(np.int64)
        c.n_rows = 2 + c.xf + 1
        c.norm = "max"
    else:
        c.geom = static_geometry(N, n_fft, hop, mode == "static_pad")
        c.rows = np.zeros(c.geom["n_frames"], np.int64)
        c.n_rows = 1
    assert not short or F_MIN <= c.geom["n_frames"] <= F_MAX
    c.gains = case_rows(_seed(case) + 50, c.n_rows, bins)
    for a in (c.x, c.gains, c.rows):
        a.setflags(write=False)
    return c


def run_ref(c, dtype=np.float64, **over):
    """``stft_ref`` on a built case -> (y, wsum, ola), y times the output scale
    (a power of two)."""
    kw = dict(c.geom, norm=c.norm, dtype=dtype)
    kw.update(over)
    win = np.hanning(c.n_fft).astype(np.float32)
    y, wsum, ola = stft_ref(c.x, win, c.gains, c.rows, **kw)
    return y * np.dtype(dtype).type(c.out_scale), wsum, ola


@functools.lru_cache(maxsize=None)
def reference(case, silent_edges=0, amp=None, N=None, gain_log2=STD_GAIN_LOG2):
    """(built case, y64, s1, s2, D) of ``case``; cached and read-only."""
    c = build(case, silent_edges, amp, N, gain_log2)
    y64, _, _ = run_ref(c)
    g = c.geom
    pos = g["out_begin"] + np.arange(g["out_len"], dtype=np.int64)
    s1, s2 = cd.window_sums(c.n_fft, c.hop, g["first_start"], g["n_frames"], pos)
    D = sample_bound(y64, s1, s2, c.n_fft, c.norm)
    for a in (y64, s1, s2, D):
        a.setflags(write=False)
    return c, y64, s1, s2, D


# ---------------------------------------------------------------------------
# float64 mutations: what the old mask could not see
# ---------------------------------------------------------------------------

def mutation_drop_last_frame_tail(c):
    """The last frame's contribution to the overlap-add dropped over its final
    ``hop`` samples (the window sum keeps it)."""
    g = c.geom
    _, wsum, ola = run_ref(c)
    _, _, ola_short = run_ref(c, n_frames=g["n_frames"] - 1)
    end = g["first_start"] + (g["n_frames"] - 1) * c.hop + c.n_fft - g["out_begin"]
    a, b = max(0, end - c.hop), min(g["out_len"], end)
    ola = ola.copy()
    ola[a:b] = ola_short[a:b]
    return ola / cd._den(wsum, c.norm)[:, None] * c.out_scale


def mutation_wsum_late(c):
    """The normaliser reads the window sum one sample late: wsum[p + 1]."""
    _, wsum, ola = run_ref(c)
    late = np.concatenate([wsum[1:], [0.0]])
    return ola / cd._den(late, c.norm)[:, None] * c.out_scale


# ---------------------------------------------------------------------------
# ragged batches and silent edges of the device test
# ---------------------------------------------------------------------------

# (mode, n_fft, hop, channels, kernel path, fused gate): three streams, one per
# tail class, in one launch
BATCHES = [("std", 2048, 512, 2, "gated 2048", True), ("std", 2048, 512, 2, "gated 2048", False),
           ("std", 4096, 1024, 2, "4096", True), ("std", 2048, 300, 1, "generic hop", True),
           ("adaptive", 2048, 512, 2, "adaptive 2048", True),
           ("static_nopad", 512, 128, 3, "static LDS pow2", True),
           ("static_pad", 100, 25, 2, "static LDS Bluestein", True)]

# digital silence over the first and last 2 n_fft samples, a loud middle
SILENT = [("std", 2048, 512, 2, "gated 2048", True), ("std", 2048, 512, 2, "gated 2048", False),
          ("xfade", 4096, 2048, 2, "4096 xfade", True),
          ("adaptive", 2048, 512, 2, "adaptive 2048", True),
          ("static_pad", 2048, 512, 2, "static 2048", True)]


def batch_id(b):
    return f"{b[0]}-{b[1]}/{b[2]}-ch{b[3]}{'' if b[5] else '-twopass'}"


def batch_cases(b):
    mode, n_fft, hop, ch, path, _ = b
    return [(mode, n_fft, hop, ch, tail, path) for tail in TAILS]


@functools.lru_cache(maxsize=None)
def batch_references(b):
    """``reference`` of the three streams of batch ``b`` with one gain table
    (the first stream's: a launch has one)."""
    cases = batch_cases(b)
    gains = build(cases[0]).gains
    out = []
    for case in cases:
        c = copy.copy(build(case))
        c.gains = gains
        y64, _, _ = run_ref(c)
        g = c.geom
        pos = g["out_begin"] + np.arange(g["out_len"], dtype=np.int64)
        s1, s2 = cd.window_sums(c.n_fft, c.hop, g["first_start"], g["n_frames"], pos)
        out.append((c, y64, s1, s2, sample_bound(y64, s1, s2, c.n_fft, c.norm)))
    return out


def silent_reference(s):
    """``reference`` of the silent-edge stream ``s`` (output gain 1: the
    limiter engages on the loud middle; the adaptive input stays below its
    attenuation threshold)."""
    mode, n_fft, hop, ch, path, _ = s
    return reference((mode, n_fft, hop, ch, "tail0", path), silent_edges=2 * n_fft,
                     amp=0.125 if mode == "adaptive" else 2.0, gain_log2=0)
