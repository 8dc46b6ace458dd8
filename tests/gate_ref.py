"""Crafted level sequences for the gate scans, and the plain automata they are
compared with (no GPU).

The device restates three sequential loops of the reference as parallel scans
(src/process_tomatis.py:373-385 standard gate, src/process_tomatis_xfade.py:
251-274 cross-fade alpha, src/process_tomatis_adaptive.py:87-121 min-hold).
The oracle has each of them as a plain loop (``gate_standard``,
``alpha_scan_xfade``, ``alpha_scan_adaptive``, ``gate_minhold``); this module
adds the standard gate on predicates in frame units, a catalogue of predicate
sequences aimed at what a scan can get wrong (run lengths around the up-delay
D, runs that mature across a thread group, a wave, a segment or a tile of
segments, all-on segments, "neither" frames that break a pending run, frames
that are "on" and "off" at once), and an alphabet of float32 ``r`` bit patterns
that realises a predicate sequence at the edges of the thresholds.

Predicates: bit 0 = level >= Ton ("on"), bit 1 = level <= Toff ("off").
"""
import functools

import numpy as np

from oracle import tomatis_oracle as orc
from tomatis_audio_processor_amd import dsp

NEI, ON, OFF, BOTH = 0, 1, 2, 3
SEG = 1024          # frames per gate segment on the device
TILE = 256          # segments per tile of the carry scan

# frame counts of the streams of one plan (odd frame_base, a stream without
# frames between others), the register-path plan, the plan with more than TILE
# segments, and the time-sharded stream
STREAM_FRAMES = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
F_REGISTER = 5000
F_TILES = TILE * SEG + SEG + 1
F_SHARDED = 9 * SEG + 77
DELAYS = (0, 1, 2, 3, 63, 64, 255, 1023, 1024, 1025, 3000)


# ---------------------------------------------------------------------------
# plain automata
# ---------------------------------------------------------------------------

def gate_frames(pred, D):
    """src/process_tomatis.py:373-385 on predicates, in frame units: frame k
    starts at sample k (hop 1) and the up-delay is D samples."""
    st = np.empty(len(pred), np.uint8)
    state, pending = 1, None
    for k, p in enumerate(np.asarray(pred).tolist()):
        if state == 1:
            if p & 1:
                if pending is None:
                    pending = k + D
            else:
                pending = None
            if pending is not None and k >= pending:
                state, pending = 2, None
        else:
            if p & 2:
                state, pending = 1, None
        st[k] = state
    return st


def pred_of_r(r, Ton, Toff):
    """The oracle's verdict on float32 ``r``: its level against Ton / Toff."""
    with np.errstate(invalid="ignore"):
        lv = orc.r_to_level(np.asarray(r, np.float32))
        return (lv >= Ton).astype(np.uint8) | ((lv <= Toff).astype(np.uint8) << 1)


def oracle_states(r, Ton, Toff, D):
    """The oracle's gate on the levels of ``r`` (frame units, as gate_frames)."""
    with np.errstate(invalid="ignore"):
        lv = orc.r_to_level(np.asarray(r, np.float32))
    return orc.gate_standard(lv, np.arange(len(lv)), Ton, Toff, D)


def xfade_rows(alpha, xf):
    """Gain row of an alpha: 0 / 1 at the ends, 2 + rint(alpha * xf) inside."""
    a = np.asarray(alpha, np.float64)
    ends = np.where(a < 0.5, 0, 1)
    if xf <= 0:
        return ends.astype(np.uint16)
    inside = (a > 0.0) & (a < 1.0)
    return np.where(inside, 2 + np.rint(a * xf).astype(np.int64), ends).astype(np.uint16)


def events(pred, D, seg=SEG):
    """What the plain automaton meets on ``pred``: counts of
    ``late``     entries whose on-run began in an earlier segment,
    ``after_nei`` entries whose on-run began right after a neither frame (the
                 entry comes exactly D frames after the run's first frame),
    ``short``    on-runs of exactly D frames (D >= 1) that end without entering,
    ``through``  entries with a whole all-on segment between run start and entry,
    and ``c2`` / ``n``, the C2 frames and all frames."""
    pred = np.asarray(pred, np.uint8).tolist()
    ev = dict(late=0, after_nei=0, short=0, through=0, c2=0, n=len(pred))
    state, pending, start = 1, None, None
    for k, p in enumerate(pred):
        if state == 1:
            if p & 1:
                if pending is None:
                    pending, start = k + D, k
            else:
                if pending is not None and k - start == D:
                    ev["short"] += 1
                pending = None
            if pending is not None and k >= pending:
                state, pending = 2, None
                ev["late"] += k // seg > start // seg
                ev["after_nei"] += start > 0 and pred[start - 1] == NEI
                ev["through"] += (start // seg + 2) * seg - 1 <= k
        else:
            if p & 2:
                state, pending = 1, None
        ev["c2"] += state == 2
    return {k: int(v) for k, v in ev.items()}


# ---------------------------------------------------------------------------
# predicate sequences
# ---------------------------------------------------------------------------

def _runs(F, lengths, classes, rng, p=None):
    out = np.empty(F, np.uint8)
    k = 0
    while k < F:
        L = int(rng.choice(lengths))
        out[k:k + L] = rng.choice(classes, p=p)
        k += L
    return out


def _placed(F, D, seg, bg, before):
    """On-runs of D and D + 1 frames whose last frame k is -1, 0, +1 mod 4, mod
    TILE and mod seg, each right after a ``before`` frame, on a ``bg``
    background; as many sequences as the runs need.  One off frame separates a
    run from the next: right after the run on an off background, two frames
    before the next run on a neither background (the gate holds C2 between)."""
    seqs, cur, last = [], None, -2
    for m in (4, TILE, seg):
        for e in (-1, 0, 1):
            for L in (D, D + 1):
                if L < 1:
                    continue
                for fresh in (False, True):
                    if cur is None or fresh:
                        if cur is not None and last >= 0:
                            seqs.append(cur)
                        cur, last = np.full(F, bg, np.uint8), -2
                    k = last + L + 2                  # first frame of the run >= max(1, last + 3)
                    k += (e - k) % m
                    if k + 1 < F:
                        a = k - L + 1
                        if a >= 2:
                            cur[a - 2 if bg == NEI else last + 1] = OFF
                        cur[a - 1] = before
                        cur[a:k + 1] = ON
                        last = k
                        break
    if cur is not None and last >= 0:
        seqs.append(cur)
    return seqs


def patterns(F, D, seg=SEG, rng=None, both=False):
    """Named predicate sequences of length F: yields (name, uint8[F])."""
    rng = np.random.default_rng(0) if rng is None else rng
    if F == 0:
        yield "empty", np.zeros(0, np.uint8)
        return
    lengths = sorted({L for L in (1, 2, D - 1, D, D + 1, D + 2, 3 * D) if 1 <= L <= F})
    # (a) random runs around D
    for i in range(3):
        yield f"a_runs{i}", _runs(F, lengths, [ON, OFF, NEI], rng, p=[0.6, 0.15, 0.25])
    # (b) runs of D and D + 1 ending around every boundary of the scan
    # (the frame before a run is off or neither; between runs the gate holds
    # C2 through neither frames either way)
    for tag, before in (("off", OFF), ("nei", NEI)):
        for i, s in enumerate(_placed(F, D, seg, NEI, before)):
            yield f"b_{tag}{i}", s
    # (c) an on-run over whole segments and one frame on either side
    for n in (1, 2, 3):
        a, b = seg - 1, (1 + n) * seg + 1           # run [a, b)
        if b + 1 <= F:
            s = np.full(F, OFF, np.uint8)
            s[a:b] = ON
            s[b + 1:] = NEI
            yield f"c_segments{n}", s
    # (d) C2, a long stretch of neither, one off frame, on again
    if F >= D + 6:
        s = np.full(F, NEI, np.uint8)
        s[0] = OFF
        s[1:D + 3] = ON
        s[max(D + 4, F - max(2, F // 4))] = OFF
        s[F - max(1, F // 8):] = ON
        yield "d_hold", s
    # (h) entered as early as can be and held: through neither to the end; to
    # one off frame at the end; on throughout after one neither frame
    if F >= D + 3:
        s = np.full(F, NEI, np.uint8)
        s[0] = OFF
        s[1:D + 2] = ON
        yield "h_hold_nei", s
        s = np.full(F, NEI, np.uint8)
        s[0:D + 1] = ON
        s[F - 1] = OFF
        yield "h_hold_off_last", s
        s = np.full(F, ON, np.uint8)
        s[0] = NEI
        yield "h_on_after_nei", s
    # (e) alternating every frame
    for tag, other in (("nei", NEI), ("off", OFF)):
        s = np.full(F, other, np.uint8)
        s[::2] = ON
        yield f"e_alt_{tag}", s
        s = np.full(F, ON, np.uint8)
        s[::2] = other
        yield f"e_alt_{tag}_odd", s
    # (f) constant
    for tag, c in (("on", ON), ("off", OFF), ("nei", NEI)):
        yield f"f_all_{tag}", np.full(F, c, np.uint8)
    if not both:
        return
    # (g) frames that are on and off at once, inside and at the ends of runs
    yield "g_all_both", np.full(F, BOTH, np.uint8)
    for i in range(3):
        yield f"g_runs{i}", _runs(F, lengths, [ON, OFF, NEI, BOTH], rng, p=[0.45, 0.1, 0.2, 0.25])
    for i in range(3):
        s = _runs(F, lengths, [ON, OFF, NEI], rng, p=[0.6, 0.15, 0.25])
        on = (s & 1).astype(bool)
        edge = np.diff(np.concatenate([[0], on.view(np.int8), [0]]))
        for a, b in zip(np.nonzero(edge == 1)[0].tolist(), np.nonzero(edge == -1)[0].tolist()):
            where = int(rng.integers(0, 6))
            k = (a - 1, a, (a + b) // 2, b - 1, b, a + min(D, b - a - 1))[where]
            if 0 <= k < F:
                s[k] = BOTH
        yield f"g_edges{i}", s
    for tag, bg in (("off", OFF), ("nei", NEI)):
        for i, s in enumerate(_placed(F, D, seg, bg, BOTH)):
            yield f"g_b_{tag}{i}", s


def tiled(F, D, seg=SEG, rng=None):
    """One sequence of F frames for a stream of more than TILE segments: the
    catalogue of whole segments (at least 4 (D + 2) frames) end to end, an on-run of D + 1 that ends on
    the first frame of segment TILE (the second tile of the carry scan) and one
    of D that ends on its last frame."""
    rng = np.random.default_rng(0) if rng is None else rng
    chunk = 4 * seg * max(1, -(-(D + 2) // seg))
    parts, n = [], 0
    while n < F:
        for _, s in patterns(chunk, D, seg, rng):
            parts.append(s)
            n += len(s)
            if n >= F:
                break
    out = np.concatenate(parts)[:F].copy()
    k = TILE * seg
    if k + seg < F and k - D - 2 >= 0:
        out[k - D - 2:k + seg + 2] = NEI
        out[k - D - 1] = OFF
        out[k - D:k + 1] = ON
        out[k + 1] = OFF
        if D >= 1 and D + 3 < seg:
            out[k + seg - D:k + seg] = ON
    return out


def shard_patterns(shards, F, D, rng=None):
    """Sequences over the F frames of a time-sharded stream, built from the
    shard bounds (timeshard.plan_shards): runs of D and D + 1 frames around
    every shard's ``b`` and ``k0``, one shard all on (with D longer than its
    summary range the entry matures shards later), one shard all neither."""
    rng = np.random.default_rng(0) if rng is None else rng
    marks = sorted({m for s in shards for m in (s.b, s.k0) if 0 < m < F})
    for L in (D, D + 1):
        if L < 1:
            continue
        for off in (-1, 0, 1, 2):
            s = np.full(F, NEI, np.uint8)
            last = -1
            for m in marks:                          # run ends at m + off
                k = m + off
                if k - L > last + 1 and k + 1 < F:
                    s[k - L] = OFF if (m + off + L) % 2 else NEI
                    s[k - L + 1:k + 1] = ON
                    s[k + 1] = OFF
                    last = k + 1
            yield f"ts_end{off:+d}_len{L}", s
    for d in sorted({-(D + 2), -(D + 1), -D, -2, -1, 0, 1, 2, D, D + 1, D + 2}):
        s = np.full(F, ON, np.uint8)                 # transitions within D + 2 of every mark
        for m in marks:
            k = m + d
            if 0 <= k < F:
                s[k] = OFF if (k & 1) else NEI
                if k + 1 < F and d % 3 == 0:
                    s[k + 1] = OFF
        yield f"ts_break{d:+d}", s
    for q, sh in enumerate(shards):
        a, b = sh.b, min(F, sh.b + sh.tf_frames)
        s = np.full(F, NEI, np.uint8)                # shard q all on, after one off frame
        s[max(0, a - 1)] = OFF
        s[a:b] = ON
        s[b:min(F, b + D + 2)] = ON if q % 2 == 0 else NEI
        if b + D + 3 < F:
            s[b + D + 3] = OFF
        yield f"ts_all_on{q}", s
        s = _runs(F, [1, 2, max(1, D), D + 1, D + 2], [ON, OFF, NEI], rng, p=[0.6, 0.15, 0.25])
        s[a:b] = NEI                                 # shard q all neither
        if a > D + 2:
            s[a - D - 2:a] = ON                      # ... entered just before it
        yield f"ts_all_nei{q}", s
    for i in range(2):
        yield f"ts_runs{i}", _runs(F, [1, 2, max(1, D - 1), max(1, D), D + 1, D + 2, 3 * D + 1],
                                   [ON, OFF, NEI], rng, p=[0.6, 0.15, 0.25])


# ---------------------------------------------------------------------------
# levels: float32 r bit patterns for a predicate sequence
# ---------------------------------------------------------------------------

_F32_ONE, _F32_INF, _F32_NAN = 0x3F800000, 0x7F800000, 0x7FC00000


class Alphabet:
    """Float32 ``r`` bit patterns at the edges of a gate's thresholds, grouped
    by the ORACLE's verdict on each (so with hysteresis <= 0 the patterns that
    are "on" and "off" at once form their own class)."""

    def __init__(self, Ton, Toff):
        self.Ton, self.Toff = Ton, Toff
        on_bits, on_exc, off_bits, off_exc = dsp.gate_bits(Ton, Toff)
        cand = [on_bits, on_bits + 1, _F32_ONE, _F32_INF,            # "on"
                off_bits, off_bits - 1, 0,                           # "off"
                on_bits - 1, off_bits + 1, _F32_NAN]                 # "neither"
        cand += list(on_exc) + list(off_exc)
        for e in list(on_exc) + list(off_exc):
            cand += [e - 1, e + 1]
        bits = np.array(sorted(set(int(b) for b in cand if 0 <= b <= _F32_NAN)), np.uint32)
        verdict = pred_of_r(bits.view(np.float32), Ton, Toff)
        self.by_class = {c: bits[verdict == c] for c in (NEI, ON, OFF, BOTH)}

    def r_bits(self, pred, rng):
        """uint32 bit patterns whose oracle verdict is ``pred`` frame by frame,
        each drawn from its class."""
        pred = np.asarray(pred, np.uint8)
        out = np.empty(len(pred), np.uint32)
        for c, pool in self.by_class.items():
            m = pred == c
            n = int(np.count_nonzero(m))
            if n:
                assert len(pool), f"no float32 level of class {c} at these thresholds"
                out[m] = pool[rng.integers(0, len(pool), n)]
        return out

    def r(self, pred, rng):
        return self.r_bits(pred, rng).view(np.float32)


def thresholds(hysteresis_db, gate_ui=50):
    T = dsp.gate_ui_to_dbfs_log_percent(gate_ui)
    return T + hysteresis_db / 2.0, T - hysteresis_db / 2.0


# ---------------------------------------------------------------------------
# cross-fade state sequences and min-hold levels
# ---------------------------------------------------------------------------

XFADES = (0, 1, 2, 47, 1023, 1024, 1500)
ASEG = 128          # frames per segment of the device's alpha scan


def xfade_state_patterns(F, xf, rng=None):
    """On / off predicate sequences (D = 0: the state follows them frame by
    frame) that flip every 1, 2, xf + 1 and xf + 2 frames, never hold a state
    for xf + 2 frames over whole alpha segments, and hold one for long."""
    rng = np.random.default_rng(0) if rng is None else rng
    if F == 0:
        yield "empty", np.zeros(0, np.uint8)
        return
    k = np.arange(F)
    for p in sorted({1, 2, xf + 1, xf + 2}):
        yield f"x_flip{p}", np.where((k // p) % 2 == 0, ON, OFF).astype(np.uint8)
        yield f"x_flip{p}_c1", np.where((k // p) % 2 == 1, ON, OFF).astype(np.uint8)
    # three alpha segments of flips shorter than xf + 2 (no frame fixes alpha),
    # between long holds
    s = np.full(F, ON, np.uint8)
    a, b = min(F, ASEG + 5), min(F, 4 * ASEG + 9)
    p = max(1, min(xf + 1, 3))
    s[a:b] = np.where(((k[a:b] - a) // p) % 2 == 0, OFF, ON)
    s[min(F, b + 2 * xf + 7):] = OFF
    yield "x_nosync", s
    lengths = sorted({L for L in (1, 2, xf, xf + 1, xf + 2, xf + 3, 2 * xf + 5) if 1 <= L <= F})
    for i in range(3):
        yield f"x_runs{i}", _runs(F, lengths, [ON, OFF, NEI], rng, p=[0.45, 0.45, 0.1])
    yield "x_all_on", np.full(F, ON, np.uint8)
    yield "x_all_off", np.full(F, OFF, np.uint8)


MINHOLDS = (0, 1, 2, 6, 1023, 1024, 1025, 5000)
MH_FRAMES = (0, 1, 5, 257, 1025, 2049, 4097, 6001, 12001)


def minhold_levels(F, mh, kind, rng, turn=0):
    """float64 levels of F frames for the min-hold gate: ``walk`` a random walk
    around the p5-p95 band, ``runs`` alternating loud / quiet plateaus that
    begin with mh - 1, mh and mh + 1 frames (in an order that ``turn`` rotates,
    so that streams too short for all three hold them between them),
    ``ties`` levels on a 0.5 dB grid with invalid frames, ``jump`` 0.35 F
    quiet, 0.55 F loud, 0.10 F quiet -- the C2 share is 0, about 0.55 or 0.65,
    or 1, never within 0.01 of a 0.5 target, so the bisection runs all its
    steps with the share on both sides of it --, ``flat`` a constant."""
    if F == 0:
        return np.zeros(0, np.float64)
    if kind == "walk":
        v = -40.0 + np.cumsum(rng.normal(0, 1.5, F))
        v -= np.linspace(0, v[-1] + 40.0, F)
        return v + rng.normal(0, 2.0, F)
    if kind == "runs":
        lengths = sorted({L for L in (1, 2, mh - 1, mh, mh + 1, mh + 2) if 1 <= L <= max(1, F)})
        lead = [L for L in (mh - 1, mh, mh + 1) if L >= 1]
        lead = lead[turn % len(lead):] + lead[:turn % len(lead)]
        out, k = np.empty(F, np.float64), 0
        hi = True
        while k < F:
            L = lead.pop(0) if lead else int(rng.choice(lengths))
            out[k:k + L] = (-25.0 if hi else -55.0) + rng.normal(0, 3.0)
            hi = not hi
            k += L
        return out
    if kind == "ties":
        v = np.repeat(rng.normal(-40, 12, F // 3 + 1), 3)[:F]
        v = np.round(v * 2) / 2
        v[rng.integers(0, F, max(1, F // 50))] = -70.0       # invalid frames
        return v
    if kind == "jump":
        v = np.full(F, -30.0)
        v[:int(round(0.35 * F))] = -50.0
        v[int(round(0.90 * F)):] = -50.0
        return v
    if kind == "flat":
        return np.full(F, -33.25)
    raise ValueError(kind)


MH_KINDS = ("walk", "runs", "ties", "jump", "flat")
MH_HYST, MH_TARGET = 3.0, 0.5


def minhold_rounds(mh):
    """Five rounds of (kinds, level arrays), one array per stream of
    MH_FRAMES; each stream meets every kind once."""
    rng = np.random.default_rng(500 + mh)
    out = []
    for j in range(len(MH_KINDS)):
        kinds = [MH_KINDS[(i + 2 * j) % len(MH_KINDS)] for i in range(len(MH_FRAMES))]
        out.append((kinds, [minhold_levels(F, mh, k, rng, turn=i)
                            for i, (F, k) in enumerate(zip(MH_FRAMES, kinds))]))
    return out


def bisection_shares(levels, mh, hyst_db=MH_HYST, target=MH_TARGET):
    """The C2 share at every threshold the oracle's bisection probes
    (src/process_tomatis_adaptive.py:133-154 as oracle.optimal_threshold walks
    it, with oracle.gate_minhold at each probe), and the threshold it returns."""
    valid = levels[levels > -70]
    lo, hi = np.percentile(valid, 5), np.percentile(valid, 95)
    best_T, best_diff, shares = np.median(valid), 1.0, []
    for _ in range(30):
        mid = (lo + hi) / 2
        st = orc.gate_minhold(levels, mid, hyst_db, mh)
        c2 = int(np.count_nonzero(st == 2)) / len(st)
        shares.append(c2)
        diff = abs(c2 - target)
        if diff < best_diff:
            best_diff, best_T = diff, mid
        if diff < 0.01:
            break
        if c2 < target:
            hi = mid
        else:
            lo = mid
    return shares, best_T


# ---------------------------------------------------------------------------
# one case through audio: block amplitudes per hop
# ---------------------------------------------------------------------------

def audio_blocks(n_blocks, D, Ton, Toff, rng):
    """Amplitude per hop block: stretches just above Ton (0.2 dB), inside the
    hysteresis band (0.5 dB under Ton) and far below Toff, with on-stretches of
    D - 1 .. D + 6 blocks (a frame spans several blocks, so the on-runs of the
    frame levels come out a few frames shorter: the caller checks what the
    oracle's levels give) and, now and then, one of 3 D blocks that enters C2,
    held through a stretch of neither and left on an off block."""
    a_on, a_nei, a_off = (10.0 ** (v / 20.0) for v in (Ton + 0.2, Ton - 0.5, Toff - 6.0))
    amps = []
    while len(amps) < n_blocks:
        kind = rng.integers(0, 8)
        if kind == 0:
            amps += [a_on] * (3 * D) + [a_nei] * int(rng.integers(5, 40)) + [a_off] * 5
        else:
            amps += [a_on] * int(rng.integers(D - 1, D + 7))
            amps += [a_nei] * int(rng.integers(4, 9)) if kind < 6 else [a_off] * 5
    return np.asarray(amps[:n_blocks], np.float32)


def square_audio(amps, hop, ch):
    """+-a square wave per hop block (every sample's square is the block's a^2)."""
    sign = np.where(np.arange(hop) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x = (np.asarray(amps, np.float32)[:, None] * sign[None, :]).reshape(-1)
    return np.repeat(x[:, None], ch, axis=1)


def oracle_frames(x, n_fft, hop):
    """(r, levels, starts) of the oracle's standard-mode frames of ``x``
    (src/process_tomatis.py:359-371 as oracle.process_standard frames them)."""
    N, ch = x.shape
    pad, pad_end, F, starts = orc._std_schedule(N, n_fft, hop)
    xpad = np.concatenate([np.zeros((pad, ch), np.float32), x, np.zeros((pad_end, ch), np.float32)])
    r = orc.frame_r(orc.frame_view(xpad, n_fft, hop, F))
    return r, orc.r_to_level(r), starts


@functools.lru_cache(maxsize=None)
def audio_case():
    """(sr, D, x, r, predicates, states): 6000 hop blocks of stereo square wave
    at 2048 / 512, 44.1 kHz, the default 250 ms up-delay, with the oracle's
    frame r, its verdicts and its gate states."""
    sr, n_fft, hop = 44100, 2048, 512
    Ton, Toff = thresholds(3.0)
    Ds = int(sr * 250.0 / 1000.0)
    D = -(-Ds // hop)
    x = square_audio(audio_blocks(6000, D, Ton, Toff, np.random.default_rng(3)), hop, 2)
    r, lv, starts = oracle_frames(x, n_fft, hop)
    states = orc.gate_standard(lv, starts, Ton, Toff, Ds)
    return sr, D, x, r, pred_of_r(r, Ton, Toff), states
