"""The crafted gate sequences of tests/gate_ref.py (no GPU): the catalogue holds
what it claims for every (frames, up-delay) pair tests/test_gpu_gate_levels.py
runs, and it detects a subtly wrong scan -- shown on the host mirror of the
kernels' run-scan algebra (timeshard.py) with one defect planted at a time."""
import numpy as np
import pytest

from oracle import tomatis_oracle as orc
from tests import gate_ref as G
from tomatis_audio_processor_amd import timeshard as T


def _total(evs):
    return {k: sum(e[k] for e in evs) for k in evs[0]}


def _sharded_N(F):
    return 16 * (F - 1) + 32          # samples giving F standard frames at 64 / 16


@pytest.mark.parametrize("hyst", [3.0, 0.0, -2.0])
def test_alphabet_classes_are_the_oracles_verdict(hyst):
    Ton, Toff = G.thresholds(hyst)
    ab = G.Alphabet(Ton, Toff)
    rng = np.random.default_rng(1)
    n_edge = 3 if hyst > 0 else 2     # (hysteresis <= 0: the bit thresholds themselves are both)
    assert len(ab.by_class[G.ON]) >= n_edge and len(ab.by_class[G.OFF]) >= n_edge
    assert len(ab.by_class[G.NEI]) >= (3 if hyst > 0 else 1)       # NaN is always neither
    assert (len(ab.by_class[G.BOTH]) > 0) == (hyst <= 0)
    for name, pred in G.patterns(300, 7, seg=64, rng=rng, both=hyst <= 0):
        r = ab.r(pred, rng)
        assert np.array_equal(G.pred_of_r(r, Ton, Toff), pred), name
        # the predicate automaton is the oracle's loop on those levels
        assert np.array_equal(G.gate_frames(pred, 7), G.oracle_states(r, Ton, Toff, 7)), name


@pytest.mark.parametrize("D", G.DELAYS)
def test_catalogue_covers_every_plan(D):
    """Per (F, D): both states in a share of 0.1 to 0.9 over the catalogue of
    that F wherever the up-delay leaves room for it.  A stream of F <= D frames
    never enters C2 (no run can last D + 1 frames: "all C1" is asserted), and
    one of D + 1 or D + 2 frames holds at most two C2 frames; an entry right
    after a neither frame and a run of D that does not enter are asserted from
    F >= D + 3 on.  At least half of the catalogue never enters by construction
    (runs of exactly D, all off, all neither, the alternations), and no member
    holds more than (F - D) / F of C2, so the share over the catalogue is at
    most (F - D) / (2 F): it is asserted where that ceiling is 0.2 or more,
    twice the bound, since members also enter late.  Of the pairs the GPU tests
    use with F >= D + 3 this leaves out (4097, 3000) alone (ceiling 0.13),
    which must still enter.  The other events are asserted where the shapes
    allow them: an entry in a later segment than its run's start needs D >= 1
    and two segments; a whole all-on segment between start and entry needs
    D >= SEG."""
    rng = np.random.default_rng(D)
    for F in G.STREAM_FRAMES + (G.F_REGISTER,):
        evs = [G.events(s, D) for _, s in G.patterns(F, D, rng=rng)]
        t = _total(evs)
        if F <= D:
            assert t["c2"] == 0
        if F >= D + 3:
            assert t["c2"] > 0, (F, D)
            if (F - D) / (2 * F) >= 0.2:
                assert 0.1 <= t["c2"] / t["n"] <= 0.9, (F, D, t)
            else:
                assert (F, D) == (4097, 3000)
            assert t["after_nei"] >= 1, (F, D, t)
            if D >= 1:
                assert t["short"] >= 1, (F, D, t)
        if D >= 1 and F >= max(2 * G.SEG, 2 * (D + 2)):
            assert t["late"] >= 1, (F, D, t)
        if D >= G.SEG and F >= D + 2 * G.SEG:
            assert t["through"] >= 1, (F, D, t)
    t = G.events(G.tiled(G.F_TILES, D, rng=rng), D)
    assert 0.1 <= t["c2"] / t["n"] <= 0.9, (D, t)
    assert t["after_nei"] >= 1 and (D == 0 or (t["short"] >= 1 and t["late"] >= 1)), (D, t)
    assert D < G.SEG or t["through"] >= 1


@pytest.mark.parametrize("world", [2, 3, 8])
def test_shard_patterns_cover_the_shard_bounds(world):
    F = G.F_SHARDED
    shards = T.plan_shards(_sharded_N(F), 64, 16, world)
    assert len(shards) == world and shards[-1].k1 == F
    for D in G.DELAYS:
        rng = np.random.default_rng(D)
        pats = list(G.shard_patterns(shards, F, D, rng))
        sts = {name: G.gate_frames(s, D) for name, s in pats}
        c2 = sum(int(np.count_nonzero(st == 2)) for st in sts.values())
        assert 0.1 <= c2 / (F * len(pats)) <= 0.9, (world, D)
        # a transition of the state within D + 2 frames of every shard's b and k0
        for sh in shards[1:]:
            for m in (sh.b, sh.k0):
                lo, hi = max(1, m - D - 2), min(F - 1, m + D + 2)
                assert any((np.diff(st[lo - 1:hi + 1].astype(np.int8)) != 0).any()
                           for st in sts.values()), (world, D, m)
        # a shard all on whose entry matures two shards later
        span = min(sh.tf_frames for sh in shards[:-1])
        if D > 2 * max(sh.tf_frames for sh in shards[:-1]) and D + span < F - shards[1].b:
            late = 0
            for q, sh in enumerate(shards):
                st = sts[f"ts_all_on{q}"]
                ent = np.nonzero(np.diff(st.astype(np.int8)) == 1)[0] + 1
                late += any(sum(1 for s2 in shards if s2.b <= k) - 1 >= q + 2 for k in ent)
            assert late >= 1, (world, D)
        for q, sh in enumerate(shards):
            a, b = sh.b, min(F, sh.b + sh.tf_frames)
            assert (dict(pats)[f"ts_all_on{q}"][a:b] == G.ON).all()
            assert (dict(pats)[f"ts_all_nei{q}"][a:b] == G.NEI).all()


@pytest.mark.parametrize("xf", G.XFADES)
def test_xfade_patterns_hold_what_they_claim(xf):
    F = 4097
    pats = dict(G.xfade_state_patterns(F, xf, np.random.default_rng(xf)))
    for p in {1, 2, xf + 1, xf + 2}:
        st = G.gate_frames(pats[f"x_flip{p}"], 0)
        runs = np.diff(np.nonzero(np.diff(st.astype(np.int8)) != 0)[0])
        assert len(runs) == 0 or (runs == p).all()
    # whole alpha segments in which no state lasts xf + 2 frames
    st = G.gate_frames(pats["x_nosync"], 0)
    a = 2 * G.ASEG
    seg = st[a - 1:3 * G.ASEG + 1]
    flips = np.nonzero(np.diff(seg.astype(np.int8)) != 0)[0]
    assert len(flips) and np.diff(np.concatenate([[0], flips, [len(seg) - 1]])).max() < xf + 2
    al = orc.alpha_scan_xfade(st, xf)
    if xf >= 2:
        assert ((al > 0) & (al < 1)).any()
    assert set(np.unique(G.xfade_rows(al, xf)).tolist()) <= set(range(0, 3 + max(0, xf)))


# ---------------------------------------------------------------------------
# the catalogue against the host mirror of the kernels' algebra, sound and
# with one defect at a time
# ---------------------------------------------------------------------------

_SEG = 64
_MIRROR_F = (1, 5, 63, 64, 65, 300)
_MIRROR_D = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 100)


def _mirror_agrees(D, F, both=False):
    """timeshard.summarize / carry_in / resolve over the catalogue, cut at
    random frames and at every segment bound, against the plain automaton."""
    rng = np.random.default_rng(1000 * D + F)
    for name, pred in G.patterns(F, D, seg=_SEG, rng=rng, both=both):
        ref = G.gate_frames(pred, D)
        if not np.array_equal(T.resolve(pred, D), ref):
            return False
        for cuts in (sorted(set(rng.integers(1, max(2, F), 4).tolist())),
                     list(range(_SEG, F, _SEG))):
            bs = [0] + [c for c in cuts if 0 < c < F] + [F]
            sums = [T.summarize(pred[a:b], D, k0=a) for a, b in zip(bs, bs[1:])]
            got = np.concatenate([T.resolve(pred[a:b], D, T.carry_in(sums, q, D), k0=a)
                                  for q, (a, b) in enumerate(zip(bs, bs[1:]))])
            if not np.array_equal(got, ref):
                return False
    return True


def test_host_mirror_equals_the_plain_automaton():
    for D in _MIRROR_D:
        for F in _MIRROR_F:
            assert _mirror_agrees(D, F), (D, F)


def _cat(X, Y, D, lead_slack=1, all_on="both", off="both"):
    NONE = T.NONE
    ao = {"both": X[0] & Y[0], "right": Y[0], "never": 0}[all_on]
    of = {"both": max(X[4], Y[4]), "left": X[4], "right": Y[4]}[off]
    if X[0]:
        return (ao, max(X[1], Y[1]), Y[2] if Y[2] != NONE else X[2], Y[3], of)
    lead = Y[2] if (Y[2] != NONE and Y[2] >= X[1] + D + lead_slack) else NONE
    return (ao, max(X[1], Y[1]), X[2], max(X[3], Y[3], lead), of)


def _apply_early(c, S, D):
    a = c[0] if S[0] else S[1]
    lead = S[2] if (S[2] != T.NONE and S[2] >= c[0] + D) else T.NONE
    return (a, max(c[1], S[3], lead), max(c[2], S[4]))


_DEFECTS = {
    "gs_apply_D": ("gs_apply", _apply_early),
    "gs_cat_D": ("gs_cat", lambda X, Y, D: _cat(X, Y, D, lead_slack=0)),
    "all_on_from_right": ("gs_cat", lambda X, Y, D: _cat(X, Y, D, all_on="right")),
    "all_on_never": ("gs_cat", lambda X, Y, D: _cat(X, Y, D, all_on="never")),
    "off_from_left": ("gs_cat", lambda X, Y, D: _cat(X, Y, D, off="left")),
    "off_from_right": ("gs_cat", lambda X, Y, D: _cat(X, Y, D, off="right")),
}


def test_sound_restatement_of_gs_cat():
    rng = np.random.default_rng(5)
    for _ in range(300):
        X, Y = (T.summarize(rng.integers(0, 3, rng.integers(1, 9)).astype(np.uint8), 3, k0=k)
                for k in (0, 9))
        assert _cat(X, Y, 3) == T.gs_cat(X, Y, 3)


@pytest.mark.parametrize("defect", sorted(_DEFECTS))
def test_catalogue_detects_a_defect_in_the_mirror(monkeypatch, defect):
    name, fn = _DEFECTS[defect]
    monkeypatch.setattr(T, name, fn)
    caught = [(D, F) for D in _MIRROR_D for F in _MIRROR_F if not _mirror_agrees(D, F)]
    assert caught, f"the catalogue passes a mirror with {defect}"
    # ... and at more than one delay: no single lucky shape
    assert len({D for D, _ in caught}) >= 3, caught


def test_audio_case_holds_runs_around_the_delay():
    """The audio case of the GPU tests, from the oracle's own frame levels:
    on-runs of D - 1 .. D + 2 frames, gaps of neither frames and gaps with off
    frames between on-runs, both states."""
    _, D, _, r, pred, states = G.audio_case()
    on = (pred & 1).astype(bool)
    edge = np.diff(np.concatenate([[0], on.view(np.int8), [0]]))
    a, b = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
    assert {D - 1, D, D + 1, D + 2} <= set((b - a).tolist())
    gaps = [pred[e:s] for e, s in zip(b[:-1], a[1:])]
    assert sum(1 for g in gaps if (g == G.NEI).all()) >= 10
    assert sum(1 for g in gaps if (g & 2).any()) >= 10
    assert 0.1 <= np.mean(states == 2) <= 0.9 and len(r) >= 5990


# ---------------------------------------------------------------------------
# min-hold level arrays
# ---------------------------------------------------------------------------

def _plateaus(v):
    """Lengths of the runs of equal values of ``v`` (the last one left out: it
    is cut at the stream's end)."""
    cuts = np.nonzero(np.diff(v) != 0)[0] + 1
    return np.diff(np.concatenate([[0], cuts])).tolist()


@pytest.mark.parametrize("mh", G.MINHOLDS)
def test_minhold_levels_hold_what_they_claim(mh):
    rounds = G.minhold_rounds(mh)
    seen = {k: [] for k in G.MH_KINDS}
    for kinds, lv in rounds:
        for F, k, v in zip(G.MH_FRAMES, kinds, lv):
            assert len(v) == F
            seen[k].append(v)
    assert all(any(len(v) >= 2049 for v in vs) for vs in seen.values()), "every kind on a long stream"
    # runs: whole plateaus of mh - 1, mh and mh + 1 frames
    want = {L for L in (mh - 1, mh, mh + 1) if L >= 1}
    assert want <= {L for v in seen["runs"] for L in _plateaus(v)}, mh
    # ties: repeated levels, and invalid frames (-70 exactly)
    for v in seen["ties"]:
        if len(v) >= 257:
            assert len(np.unique(v)) < len(v) // 2 and (v == -70.0).any() and (v > -70).any()
    # jump: the bisection probes shares on both sides of the target and never
    # within 0.01 of it, so it runs its 30 steps
    for v in seen["jump"]:
        if len(v) >= 5:
            shares, T = G.bisection_shares(v, mh)
            assert T == orc.optimal_threshold(v, v > -70, G.MH_HYST, mh, G.MH_TARGET)
            assert len(shares) == 30 and min(shares) < G.MH_TARGET < max(shares), (mh, len(v))
            assert min(abs(c - G.MH_TARGET) for c in shares) >= 0.01, (mh, len(v), shares)
    # flat: one side only (the other kind of stream that never converges)
    for v in seen["flat"]:
        if len(v) >= 5:
            assert len(G.bisection_shares(v, mh)[0]) == 30
