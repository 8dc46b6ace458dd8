"""The calibration automaton of tests/cal_ref.py (no GPU): anchored on the
oracle's gate, on the frame-unit gate of tests/gate_ref.py and on the
reference's own golden run; its vectorised grid and search against the scalar
loop and the golden JSON; what the catalogue holds; and that the catalogue
catches every planted defect."""
import json

import numpy as np
import pytest

from oracle import tomatis_oracle as orc
from tests import cal_ref as R
from tests import gate_ref as G
from tests.test_calibration import fixture


def _small(c):
    return c.F <= 5


def test_threshold_comparison_is_float32():
    """NEP 50: an np.float32 level against the Python float T +- hyst / 2 is
    compared in float32.  The automaton (Python-float thresholds) equals the
    oracle's loop on Python-float levels against the thresholds rounded to
    float32 -- on every case -- and hyst 0.3 holds a level that the unrounded
    double threshold would judge the other way."""
    cat, st = R.catalogue(), R.catalogue_states()
    for c, s in zip(cat, st):
        t_on, t_off = R.thresholds32(R.T_CASE, c.hyst)
        want = orc.gate_standard(c.levels, c.starts, float(t_on), float(t_off), c.up)
        assert np.array_equal(s, want), (c.name, c.hyst, c.F, c.D, c.kind, c.up)
    flips = 0
    for hyst in R.HYSTS:
        t_on, t_off = R.thresholds32(R.T_CASE, hyst)
        flips += (float(t_on) >= R.T_CASE + hyst / 2) != (t_on >= R.T_CASE + hyst / 2)
        flips += (float(t_off) <= R.T_CASE - hyst / 2) != (t_off <= R.T_CASE - hyst / 2)
    assert flips >= 1, "no threshold of the catalogue tells float32 from double comparison"


def test_alphabet_classes():
    for hyst in R.HYSTS:
        ab = R.alphabet(R.T_CASE, hyst)
        assert len(ab[G.ON]) >= 2 and len(ab[G.OFF]) >= 2
        assert (len(ab[G.NEI]) == 3) == (hyst > 0) and (len(ab[G.BOTH]) == 1) == (hyst == 0)
        for c, pool in ab.items():
            assert np.all(R.verdict(pool, R.T_CASE, hyst) == c), (hyst, c)


def test_even_starts_are_the_frame_gate():
    """On evenly spaced starts an up-delay of ``up`` samples is one of
    ceil(up / hop) frames."""
    n = 0
    for c, s in zip(R.catalogue(), R.catalogue_states()):
        if c.kind == "even":
            pred = R.verdict(c.levels, R.T_CASE, c.hyst)
            assert np.array_equal(s, G.gate_frames(pred, -(-c.up // R.HOP))), (c.name, c[1:5], c.up)
            n += 1
    assert n > 1000


def test_golden_sim_states():
    fx = fixture()
    fit = np.flatnonzero(fx["music_mask"])
    fs = (np.arange(len(fx["orig_level"])) * 2048).astype(np.int64)[fit]
    assert np.any(np.diff(fs) > 2048), "the golden's fitted frames have gaps"
    for (g, T, hy, up), ref in zip(fx["sim_params"], fx["sim_states"]):
        lv = (fx["orig_level"] + np.float32(g))[fit]
        assert np.array_equal(R.states(lv, fs, T, hy, up, 48000), ref)


def test_grid_counts_equal_the_scalar_loop():
    cat, st = R.catalogue(), R.catalogue_states()
    seen = 0
    for l in R.launches():
        if l.F > 5:
            continue
        cnt, s = R.grid_counts(l.rows, l.starts, l.target, l.cands, want_states=True)
        assert cnt.shape == (len(l.cands), 2) and s.shape == (len(l.cands), l.F)
        for j, i in enumerate(l.index):
            assert np.array_equal(s[j], st[i]), (cat[i].name, cat[i][1:5])
            assert tuple(cnt[j]) == R.counts(st[i], l.target)
            seen += 1
        no_target = R.grid_counts(l.rows, l.starts, None, l.cands)
        assert not no_target[:, 0].any() and np.array_equal(no_target[:, 1], cnt[:, 1])
    assert seen == sum(1 for c in cat if _small(c))


def test_grid_counts_equal_the_scalar_loop_on_long_cases():
    """One launch of 257 and of 700 gapped frames."""
    cat, st = R.catalogue(), R.catalogue_states()
    for F in (257, 700):
        l = next(l for l in R.launches() if l.F == F and cat[l.index[0]].kind == "gapped")
        cnt, s = R.grid_counts(l.rows, l.starts, l.target, l.cands, want_states=True)
        for j, i in enumerate(l.index):
            assert np.array_equal(s[j], st[i]), (cat[i].name, cat[i][1:5])
            assert tuple(cnt[j]) == R.counts(st[i], l.target)


def test_search_reproduces_the_golden_json():
    fx = fixture()
    js = json.loads(str(fx["json"]))
    fs = (np.arange(len(fx["orig_level"])) * 2048).astype(np.int64)
    best, gain_db0, n = R.search(fx["orig_level"], fx["base_level"], fx["base_state"],
                                 fx["music_mask"], fs, 48000)
    assert n == 13 * 6 * 6 * 81
    assert best["T"] == js["T_adj_dbfs"] and best["hyst"] == js["hyst_db"]
    assert best["up_ms"] == js["up_delay_ms"] and best["gain_db"] == js["gain_db_base_minus_orig"]
    assert best["mismatch"] == js["mismatch"] and best["switches"] == js["switches"]


def test_catalogue_conditions():
    """Every (hyst, F >= D + 3, D) group holds a case with a C2 share in
    [0.1, 0.9] on even and on gapped starts, and for D >= 2 a gapped case
    whose states differ from those of the same levels and delay on even
    starts (a gap has jumped over ``pending``)."""
    cat, st = R.catalogue(), R.catalogue_states()
    even = {(id(c.levels), c.up): s for c, s in zip(cat, st) if c.kind == "even"}
    mixed, moved, groups = set(), set(), set()
    for c, s in zip(cat, st):
        if c.F < c.D + 3:
            continue
        g = (c.hyst, c.F, c.D)
        groups.add(g)
        if 0.1 <= np.mean(s == 2) <= 0.9:
            mixed.add(g + (c.kind,))
        if c.kind == "gapped" and not np.array_equal(s, even[(id(c.levels), c.up)]):
            moved.add(g)
    assert len(groups) == len(R.HYSTS) * sum(F >= D + 3 for F in R.FRAMES for D in R.DELAYS)
    for g in sorted(groups):
        assert g + ("even",) in mixed and g + ("gapped",) in mixed, g
        if g[2] >= 2:
            assert g in moved, g
    # delays that are no multiple of the hop, and the zero delay entering at once
    assert any(c.up % R.HOP for c in cat) and any(c.up == 0 and s[:1].tolist() == [2]
                                                  for c, s in zip(cat, st))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_planted_defect_is_caught(variant):
    """Each defect changes the states, or the counts against an all-C1 target,
    of at least one case; and on gapped starts for the defects that only gaps
    can show."""
    cat, st = R.catalogue(), R.catalogue_states()
    kinds = set()
    for c, s in zip(cat, st):
        if c.kind in kinds:
            continue
        got = R.truth(c, variant)
        target = np.ones(c.F, np.int32)
        if not np.array_equal(got, s) or R.counts(got, target, variant) != R.counts(s, target):
            kinds.add(c.kind)
        if len(kinds) == 2:
            break
    assert kinds, variant
    if variant == "pending_frames":
        assert "gapped" in kinds
