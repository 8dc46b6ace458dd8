"""The gate-calibration automaton as a plain statement, its vectorised grid,
the search built on it, and the crafted cases the calibration grid is judged
on (no GPU; tests/test_cal_ref.py on the CPU, tests/test_gpu_cal_grid.py on
the device).

The rule (src/calibrate_to_baseline_v2.py:84-109): the gate starts in C1.  In
C1 a frame whose level is >= Ton arms ``pending = start + up_delay`` unless one
is armed already, any other frame disarms it, and the gate enters C2 on the
first frame whose start has reached an armed ``pending`` (that frame itself
when the delay is 0), disarming it.  In C2 a frame whose level is <= Toff goes
back to C1.  ``up_delay = int(round(sr * up_ms / 1000))`` samples; Ton / Toff
are the Python floats ``T +- hyst / 2`` and the levels numpy float32 scalars,
so the comparison is whatever numpy makes of that pair (NEP 50: float32).

Unlike the processors' gate (tests/gate_ref.py, evenly spaced frames) the
calibration fits music-masked frames only: the starts have gaps, so a delay is
a number of samples, not of frames.

``states(..., variant=...)`` plants one defect at a time (VARIANTS);
tests/test_cal_ref.py shows that the catalogue catches each of them.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import gate_ref as G
from tomatis_audio_processor_amd._lib import GATE_CAND_DTYPE

SR = 48000
HOP = 2048
T_CASE = -37.123
HYSTS = (0.0, 0.3, 1.0, 6.0)
FRAMES = (0, 1, 2, 5, 257, 700)
DELAYS = (0, 1, 2, 3, 7)          # up-delays in frames of HOP
SEG = 64

VARIANTS = (
    "st_gt_pending",    # enters on st > pending
    "lv_gt_ton",        # arms on lv > Ton
    "lv_lt_toff",       # leaves on lv < Toff
    "pending_kept",     # pending survives C2: the next on-frame after leaving enters at once
    "pending_frames",   # the delay counted in frames (ceil(up / hop)) of the fitted sequence
    "switch_frame0",    # the switch count compares frame 0 with the initial C1
    "thr_f32_sum",      # thresholds rounded as float32(T) +- float32(hyst / 2); at T_CASE
                        # and hyst 0.3 that moves Toff by one ulp (and leaves Ton alone)
)


# ---------------------------------------------------------------------------
# the sequential automaton
# ---------------------------------------------------------------------------

def up_samples(up_ms, sr):
    return int(round(sr * up_ms / 1000.0))


def states(levels_f32, starts_i64, T, hyst, up_ms, sr, variant=None, hop=HOP):
    """int32 states (1 / 2) of the automaton over float32 levels and int64
    frame starts.  ``hop`` only serves the ``pending_frames`` variant.

    ``pending_kept``: in the true rule pending is disarmed both on entering and
    on leaving C2, and either reset alone is enough (nothing arms it inside
    C2); the variant drops both."""
    assert variant is None or variant in VARIANTS, variant
    levels = np.asarray(levels_f32)
    assert levels.dtype == np.float32
    t_on = float(T) + float(hyst) / 2
    t_off = float(T) - float(hyst) / 2
    if variant == "thr_f32_sum":
        t_on = float(np.float32(T) + np.float32(float(hyst) / 2))
        t_off = float(np.float32(T) - np.float32(float(hyst) / 2))
    up = up_samples(up_ms, sr)
    by_frames = variant == "pending_frames"
    if by_frames:
        up = -(-up // hop)
    out = np.empty(len(levels), np.int32)
    state, pending = 1, None
    for i, (lv, st) in enumerate(zip(levels, np.asarray(starts_i64, np.int64).tolist())):
        now = i if by_frames else st
        if state == 1:
            on = lv > t_on if variant == "lv_gt_ton" else lv >= t_on
            if on:
                if pending is None:
                    pending = now + up
            else:
                pending = None
            if pending is not None and (now > pending if variant == "st_gt_pending"
                                        else now >= pending):
                state = 2
                if variant != "pending_kept":
                    pending = None
        else:
            off = lv < t_off if variant == "lv_lt_toff" else lv <= t_off
            if off:
                state = 1
                if variant != "pending_kept":
                    pending = None
        out[i] = state
    return out


def counts(st, target, variant=None):
    """(mismatch, switches): frames whose state differs from ``target`` (0
    without a target) and frames i >= 1 whose state differs from frame i - 1."""
    st = np.asarray(st)
    mis = 0 if target is None else int(np.count_nonzero(st != np.asarray(target)))
    sw = int(np.count_nonzero(st[1:] != st[:-1]))
    if variant == "switch_frame0" and len(st):
        sw += int(st[0] != 1)
    return mis, sw


# ---------------------------------------------------------------------------
# all candidates at once
# ---------------------------------------------------------------------------

def cand_table(rows, Ts, hysts, ups_ms, sr):
    """Candidate records (the device's TomatisGateCand) for equally long
    sequences of level row, T, hyst and up-delay: thresholds rounded to float32
    once, T +- hyst / 2 formed in double."""
    n = len(rows)
    c = np.zeros(n, GATE_CAND_DTYPE)
    c["level_row"] = rows
    T = np.asarray(Ts, np.float64)
    h = np.asarray(hysts, np.float64)
    c["t_on"] = (T + h / 2).astype(np.float32)
    c["t_off"] = (T - h / 2).astype(np.float32)
    c["up_delay"] = [up_samples(float(u), sr) for u in ups_ms]
    return c


def grid_counts(level_rows, starts, target, cands, want_states=False):
    """The automaton for every candidate: a loop over frames, numpy over
    candidates.  -> int32 [n_cand, 2] (mismatch, switches) and, on request, the
    uint8 states [n_cand, n_fit]."""
    lv = np.asarray(level_rows, np.float32)
    if lv.ndim == 1:
        lv = lv[None, :]
    starts = np.asarray(starts, np.int64)
    n_fit, n = len(starts), len(cands)
    row = np.asarray(cands["level_row"], np.int64)
    t_on = np.asarray(cands["t_on"], np.float32)
    t_off = np.asarray(cands["t_off"], np.float32)
    up = np.asarray(cands["up_delay"], np.int64)
    c2 = np.zeros(n, bool)
    armed = np.zeros(n, bool)
    pending = np.zeros(n, np.int64)
    prev = np.zeros(n, bool)
    mis = np.zeros(n, np.int32)
    sw = np.zeros(n, np.int32)
    out = np.empty((n, n_fit), np.uint8) if want_states else None
    for i in range(n_fit):
        l = lv[row, i]
        st = starts[i]
        on, off = l >= t_on, l <= t_off
        c1 = ~c2
        arm = c1 & on & ~armed
        pending[arm] = st + up[arm]
        armed = c1 & on
        enter = armed & (st >= pending)
        leave = c2 & off
        c2 = (c2 | enter) & ~leave
        armed &= ~enter
        if target is not None:
            mis += c2 != (target[i] == 2)
        if i > 0:
            sw += c2 != prev
        prev = c2.copy()
        if want_states:
            out[:, i] = 1 + c2
    cnt = np.stack([mis, sw], axis=1)
    return (cnt, out) if want_states else cnt


# ---------------------------------------------------------------------------
# the search (src/calibrate_to_baseline_v2.py:227-265)
# ---------------------------------------------------------------------------

DEFAULT_DELAYS_MS = (0, 50, 100, 150, 200, 250)
DEFAULT_HYSTS = (0, 1, 2, 3, 4, 6)


def search_table(orig_level, base_level, base_state, music_mask, frame_starts, sr, *,
                 gain_search_pm_db=3.0, gain_step_db=0.5, T_pm_db=10.0, T_step_db=0.25,
                 delay_list_ms=DEFAULT_DELAYS_MS, hyst_list=DEFAULT_HYSTS):
    """The candidates of the search in its loop order: gains around the median
    level difference of the music frames (float32 steps), per gain -- skipped
    when the target holds fewer than 10 fitted frames of either state -- the
    up-delays, inside them the hystereses, inside them the thresholds around
    the mean of the two classes' median levels (float32 steps).
    -> (rows, fitted starts, fitted target, cands, meta, gain_db0)."""
    mm = np.asarray(music_mask, bool)
    gain_db0 = float(np.median((base_level - orig_level)[mm]))
    gains = np.arange(gain_db0 - gain_search_pm_db, gain_db0 + gain_search_pm_db + 1e-9,
                      gain_step_db).astype(np.float32)
    fit = np.flatnonzero(mm)
    fs_fit, s_fit = np.asarray(frame_starts)[fit], np.asarray(base_state)[fit]
    rows, meta = [], []
    for g in gains:
        adj = (orig_level + g)[fit]
        lo, hi = adj[s_fit == 1], adj[s_fit == 2]
        if len(lo) < 10 or len(hi) < 10:
            continue
        T0 = 0.5 * (float(np.median(lo)) + float(np.median(hi)))
        Ts = np.arange(T0 - T_pm_db, T0 + T_pm_db + 1e-9, T_step_db).astype(np.float32)
        rows.append(adj)
        for up_ms in delay_list_ms:
            for hyst in hyst_list:
                for T in Ts:
                    meta.append((len(rows) - 1, float(T), float(hyst), float(up_ms), float(g),
                                 float(T0)))
    if not meta:
        return None, fs_fit, s_fit, None, meta, gain_db0
    r, T, h, u = (np.array([m[j] for m in meta]) for j in range(4))
    return np.stack(rows), fs_fit, s_fit, cand_table(r.astype(np.int64), T, h, u, sr), meta, gain_db0


def pick(meta, cnt, n_fit):
    """The reference's score and its first strict minimum in loop order."""
    best = None
    for (_, T, hyst, up_ms, g, T0), (mis, sw) in zip(meta, np.asarray(cnt).tolist()):
        mismatch = float(mis / n_fit)
        score = mismatch + 1e-5 * sw
        if best is None or score < best["score"]:
            best = dict(score=score, mismatch=mismatch, switches=int(sw), T=T, hyst=hyst,
                        up_ms=up_ms, gain_db=g, T0=T0)
    return best


def search(orig_level, base_level, base_state, music_mask, frame_starts, sr, **kw):
    """-> (best dict or None, gain_db0, number of candidates)."""
    rows, fs_fit, s_fit, cands, meta, gain_db0 = search_table(
        orig_level, base_level, base_state, music_mask, frame_starts, sr, **kw)
    if not meta:
        return None, gain_db0, 0
    return pick(meta, grid_counts(rows, fs_fit, s_fit, cands), len(s_fit)), gain_db0, len(meta)


# ---------------------------------------------------------------------------
# levels at the edges of float32 thresholds
# ---------------------------------------------------------------------------

def thresholds32(T, hyst):
    return np.float32(float(T) + float(hyst) / 2), np.float32(float(T) - float(hyst) / 2)


def alphabet(T, hyst):
    """{class: float32 levels} around float32(T +- hyst / 2): the threshold
    itself, its float32 neighbour on the far side and a far value for on and
    off; the neighbours on the near side and the middle for neither (hyst > 0
    only); the one threshold for both (hyst == 0 only, where it is not in the
    on and off classes)."""
    t_on, t_off = thresholds32(T, hyst)
    inf = np.float32(np.inf)
    on = [t_on, np.nextafter(t_on, inf), t_on + np.float32(40)]
    off = [t_off, np.nextafter(t_off, -inf), t_off - np.float32(40)]
    nei, both = [], []
    if hyst > 0:
        assert np.nextafter(t_off, inf) < t_on
        nei = [np.nextafter(t_on, -inf), np.nextafter(t_off, inf),
               np.float32((float(t_on) + float(t_off)) / 2)]
    else:
        assert t_on == t_off
        both, on, off = [t_on], on[1:], off[1:]
    return {G.ON: np.array(on, np.float32), G.OFF: np.array(off, np.float32),
            G.NEI: np.array(nei, np.float32), G.BOTH: np.array(both, np.float32)}


def verdict(levels, T, hyst):
    """Predicates of float32 levels against the float32 thresholds."""
    t_on, t_off = thresholds32(T, hyst)
    lv = np.asarray(levels, np.float32)
    return (lv >= t_on).astype(np.uint8) | ((lv <= t_off).astype(np.uint8) << 1)


def levels_of(pred, ab, rng):
    """float32 levels drawn from the classes of ``pred``; without neither
    levels (hyst == 0) a neither frame is an off frame."""
    pred = np.asarray(pred, np.uint8)
    if len(ab[G.NEI]) == 0:
        pred = np.where(pred == G.NEI, G.OFF, pred)
    out = np.empty(len(pred), np.float32)
    for c, pool in ab.items():
        m = pred == c
        k = int(np.count_nonzero(m))
        if k:
            assert len(pool), f"no level of class {c}"
            out[m] = pool[rng.integers(0, len(pool), k)]
    return out


# ---------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------

# name, hyst, F, D, kind ("even" / "gapped"), levels, starts, up_ms, up (samples)
Case = namedtuple("Case", "name hyst F D kind levels starts up_ms up")


@functools.lru_cache(maxsize=None)
def even_starts(F):
    return np.arange(F, dtype=np.int64) * HOP


@functools.lru_cache(maxsize=None)
def gapped_starts(F, D):
    """Starts of F fitted frames: a random 70 % of the frames 0 .. F / 0.7 of
    hop HOP, frame 0 among them."""
    if F == 0:
        return np.zeros(0, np.int64)
    n = max(F, int(round(F / 0.7)))
    rng = np.random.default_rng(1000 * F + D)
    rest = np.sort(rng.choice(np.arange(1, n), F - 1, replace=False)) if F > 1 else []
    return np.concatenate([[0], rest]).astype(np.int64) * HOP


def _ms(up):
    up_ms = up * 1000.0 / SR
    assert up_samples(up_ms, SR) == up
    return up_ms


@functools.lru_cache(maxsize=None)
def catalogue():
    """Every case: per (hyst, F, D) the predicate sequences of
    gate_ref.patterns as levels of the alphabet, on even starts with up-delays
    of D hops - 1, D hops and D hops + 1 samples (no negative delay) and on
    gapped starts with D hops and D hops + 1 samples."""
    out = []
    for hyst in HYSTS:
        ab = alphabet(T_CASE, hyst)
        for F in FRAMES:
            for D in DELAYS:
                rng = np.random.default_rng(int(10 * hyst) * 10007 + 101 * F + D)
                ev, gp = even_starts(F), gapped_starts(F, D)
                for name, pred in G.patterns(F, D, seg=SEG, rng=rng, both=(hyst == 0)):
                    lv = levels_of(pred, ab, rng)
                    for up in (D * HOP - 1, D * HOP, D * HOP + 1):
                        if up >= 0:
                            out.append(Case(name, hyst, F, D, "even", lv, ev, _ms(up), up))
                    for up in (D * HOP, D * HOP + 1):
                        out.append(Case(name, hyst, F, D, "gapped", lv, gp, _ms(up), up))
    return out


def truth(case, variant=None):
    return states(case.levels, case.starts, T_CASE, case.hyst, case.up_ms, SR, variant=variant)


@functools.lru_cache(maxsize=None)
def catalogue_states():
    """The sequential automaton's states of every catalogue case (computed
    once, shared, never modified)."""
    out = [truth(c) for c in catalogue()]
    for s in out:
        s.flags.writeable = False
    return out


Launch = namedtuple("Launch", "F starts target rows cands index")


@functools.lru_cache(maxsize=None)
def launches():
    """The catalogue as device launches: the cases that share a starts array
    are the candidates of one launch, their distinct level arrays its rows.
    ``index[j]`` is the catalogue index of candidate j; the target is a random
    1 / 2 sequence."""
    cat = catalogue()
    groups = {}
    for i, c in enumerate(cat):
        groups.setdefault((c.F, id(c.starts)), []).append(i)
    out = []
    for k, ((F, _), idx) in enumerate(groups.items()):
        rng = np.random.default_rng(77 + k)
        row_of, rows = {}, []
        for i in idx:
            if id(cat[i].levels) not in row_of:
                row_of[id(cat[i].levels)] = len(rows)
                rows.append(cat[i].levels)
        cands = cand_table([row_of[id(cat[i].levels)] for i in idx], [T_CASE] * len(idx),
                           [cat[i].hyst for i in idx], [cat[i].up_ms for i in idx], SR)
        target = rng.integers(1, 3, F).astype(np.int32)
        out.append(Launch(F, cat[idx[0]].starts, target,
                          np.stack(rows).reshape(len(rows), F), cands, tuple(idx)))
    return out
