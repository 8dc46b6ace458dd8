"""GPU: the gate-calibration grid and the band energies against their plain
statements (tests/cal_ref.py; what its catalogue holds and that it catches a
subtly wrong automaton is shown on the CPU in tests/test_cal_ref.py).

Grid (tomatis_cal_gate_grid through calibrate_to_baseline_v2._grid, exact): the
states and both counts of every catalogue case -- float32 levels at the edges
of float32 thresholds, evenly spaced and gapped frame starts, up-delays that
are no multiple of the hop -- against the sequential automaton; candidate
indexing across 256-lane workgroups with level rows out of order; the ABI's
edges; the whole default grid (37,908 candidates) at the golden's size; and
simulate_state / search_grid against cal_ref.states / cal_ref.search.

Band energies (tomatis_an_band_energy, k_an_band_pair): per (frame, band) the
float64 value of sum |rfft(hanning * power_mono(frame))|^2 over the band;

    e   = largest relative error of the device's float32 sums,
    e32 = the same for the formula in float32 numpy (scipy.fft.rfft on float32,
          float32 power, float32 sum),
    e  <= FACTOR * max(e32, 2^-23),   FACTOR = 8

(tests/stft_ref.py: bound), over the frames and the two bands of one call.
FACTOR holds at every size, the power-of-two 16384 included: the ceiling
factor that tests/test_gpu_spectral_fidelity.py needs for single bins of a
power-mono spectrum at n_fft >= 8192 is not needed for these sums (the one-bin
bands here, N/4 and N/2, measure 1.00 at the powers of two: e and e32 agree to
four digits there).

Largest measured e / max(e32, 2^-23) per path on the MI355X:

    band pow2        2.20   (16384/8192, 2 frames, overlapping bands)
    band Bluestein   2.97   (100/37: 1 frame, one-bin band; 5 frames, touching bands)
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from tests import cal_ref as R
from tests.stft_ref import FACTOR, FLOOR, bound, white
from tests.test_calibration import fixture

pytestmark = pytest.mark.gpu
SR = 48000
EPS = 1e-12


def _cal():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import calibrate_to_baseline_v2 as cal
    return torch, cal


def _L():
    from tomatis_audio_processor_amd import _lib
    return _lib


# ---------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------

def test_catalogue_states_and_counts():
    """Every catalogue case as one candidate of its launch: states, mismatches
    against a random target and switches equal the sequential automaton's."""
    _, cal = _cal()
    cat, want = R.catalogue(), R.catalogue_states()
    seen = 0
    for l in R.launches():
        cnt, st = cal._grid(l.rows, l.starts, l.target, l.cands, want_states=True)
        assert cnt.shape == (len(l.cands), 2) and st.shape == (len(l.cands), l.F)
        for j, i in enumerate(l.index):
            c = cat[i]
            assert np.array_equal(st[j], want[i]), (c.name, c.hyst, c.F, c.D, c.kind, c.up)
            assert tuple(cnt[j].tolist()) == R.counts(want[i], l.target), \
                (c.name, c.hyst, c.F, c.D, c.kind, c.up)
            seen += 1
    assert seen == len(cat)


@pytest.mark.parametrize("n_cand", [0, 1, 255, 256, 257, 1000])
def test_candidate_indexing(n_cand):
    """Candidate c reads its own record and its own level row (rows assigned
    out of order) and writes row c of [n_cand][n_fit] and out[2c], out[2c+1]."""
    _, cal = _cal()
    rng = np.random.default_rng(5)
    n_fit = 41
    rows = rng.normal(-37.0, 3.0, (3, n_fit)).astype(np.float32)
    starts = R.gapped_starts(n_fit, 0)
    target = rng.integers(1, 3, n_fit).astype(np.int32)
    c = np.arange(n_cand)
    cands = R.cand_table((5 * c + 2) % 3, -40.0 + 0.07 * (c % 97), np.take(R.HYSTS, c % 4),
                         (c % 5) * 1000 * 1000.0 / SR, SR)
    want_cnt, want_st = R.grid_counts(rows, starts, target, cands, want_states=True)
    cnt, st = cal._grid(rows, starts, target, cands, want_states=True)
    assert cnt.shape == (n_cand, 2) and st.shape == (n_cand, n_fit)
    assert np.array_equal(st, want_st)
    assert np.array_equal(cnt, want_cnt)
    if n_cand > 3:
        # the truth tells a wrong row or a wrong candidate apart
        moved = cands.copy()
        moved["level_row"] = (moved["level_row"] + 1) % 3
        assert not np.array_equal(R.grid_counts(rows, starts, target, moved), want_cnt)
        assert len(np.unique(want_st, axis=0)) > min(n_cand, 97) // 2
    for j in range(0, n_cand, 131):     # and the scalar loop itself on a few
        s = R.states(rows[cands["level_row"][j]], starts, -40.0 + 0.07 * (j % 97),
                     R.HYSTS[j % 4], (j % 5) * 1000 * 1000.0 / SR, SR)
        assert np.array_equal(st[j], s) and tuple(cnt[j].tolist()) == R.counts(s, target)


def test_no_frames_and_no_target():
    _, cal = _cal()
    cands = R.cand_table([0, 0, 0], [-37.0, -30.0, -20.0], [0, 1, 6], [0, 50, 100], SR)
    cnt, st = cal._grid(np.zeros((1, 0), np.float32), np.zeros(0, np.int64),
                        np.zeros(0, np.int32), cands, want_states=True)
    assert cnt.tolist() == [[0, 0]] * 3 and st.shape == (3, 0)
    l = next(l for l in R.launches() if l.F == 257)
    cnt, st = cal._grid(l.rows, l.starts, None, l.cands, want_states=True)
    want = R.grid_counts(l.rows, l.starts, None, l.cands)
    assert not cnt[:, 0].any() and np.array_equal(cnt, want) and want[:, 1].any()


def test_grid_argument_errors():
    """TOMATIS_E_ARG before any launch: nothing is written."""
    torch, _ = _cal()
    lib = _L()
    L, ptr, hs = lib.lib(), lib.ptr, lib.stream_handle()
    n_fit, n_cand = 8, 4
    lv = torch.zeros(n_fit, dtype=torch.float32, device="cuda")
    st = torch.arange(n_fit, dtype=torch.int64, device="cuda")
    cb = torch.from_numpy(R.cand_table([0] * n_cand, [-1.0] * n_cand, [0] * n_cand,
                                       [0] * n_cand, SR).view(np.uint8)).cuda()
    out = torch.full((n_cand, 2), -7, dtype=torch.int32, device="cuda")
    null = C.c_void_p(0)
    bad = [
        (ptr(lv), -1, ptr(st), ptr(cb), n_cand, ptr(out)),
        (ptr(lv), n_fit, ptr(st), ptr(cb), -1, ptr(out)),
        (ptr(lv), n_fit, ptr(st), null, n_cand, ptr(out)),
        (ptr(lv), n_fit, ptr(st), ptr(cb), n_cand, null),
        (null, n_fit, ptr(st), ptr(cb), n_cand, ptr(out)),
        (ptr(lv), n_fit, null, ptr(cb), n_cand, ptr(out)),
    ]
    for levels, nf, starts, cands, nc, o in bad:
        rc = L.tomatis_cal_gate_grid(levels, nf, starts, null, cands, nc, o, null, hs)
        assert rc == lib.E_ARG, (nf, nc)
    # no candidates: nothing to do, whatever the other pointers are
    assert L.tomatis_cal_gate_grid(null, 0, null, null, null, 0, null, null, hs) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())


@functools.lru_cache(maxsize=None)
def _golden_table():
    fx = fixture()
    fs = (np.arange(len(fx["orig_level"])) * 2048).astype(np.int64)
    rows, fs_fit, s_fit, cands, meta, g0 = R.search_table(
        fx["orig_level"], fx["base_level"], fx["base_state"], fx["music_mask"], fs, SR)
    want = R.grid_counts(rows, fs_fit, s_fit, cands)
    return fx, fs, rows, fs_fit, s_fit, cands, (meta, g0), want


def test_default_grid_full_count_table():
    """13 gains x 6 up-delays x 6 hystereses x 81 thresholds over the golden's
    761 fitted frames: every candidate's two counts."""
    _, cal = _cal()
    fx, fs, rows, fs_fit, s_fit, cands, (meta, _), want = _golden_table()
    assert len(cands) == 37908 and rows.shape == (13, len(fs_fit))
    cnt, _ = cal._grid(rows, fs_fit, s_fit, cands)
    bad = np.flatnonzero((cnt != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], [meta[i] for i in bad[:5]])


def test_search_grid_on_the_golden():
    _, cal = _cal()
    fx, fs, rows, fs_fit, s_fit, cands, (meta, gain_db0), want = _golden_table()
    got = cal.search_grid(fx["orig_level"], fx["base_state"], fx["music_mask"], fs, SR,
                          base_level=fx["base_level"])
    assert got == (R.pick(meta, want, len(s_fit)), gain_db0, 37908)
    js = json.loads(str(fx["json"]))
    assert got[0]["T"] == js["T_adj_dbfs"] and got[0]["switches"] == js["switches"]


# ---------------------------------------------------------------------------
# simulate_state and search_grid
# ---------------------------------------------------------------------------

def test_simulate_state_on_the_catalogue():
    """Every 37th case, and every case of at most two frames (the empty
    sequence among them)."""
    _, cal = _cal()
    cat, want = R.catalogue(), R.catalogue_states()
    n = 0
    for i, c in enumerate(cat):
        if i % 37 and (c.F > 2 or i % 5):
            continue
        got = cal.simulate_state(c.levels, c.starts, SR, R.T_CASE, c.hyst, c.up_ms)
        assert got.dtype == np.int32 and got.shape == (c.F,)
        assert np.array_equal(got, want[i]), (c.name, c.hyst, c.F, c.D, c.kind, c.up)
        n += 1
    assert n > 300
    assert cal.simulate_state(np.zeros(0, np.float32), np.zeros(0, np.int64), SR, -30.0, 2.0,
                              100.0).shape == (0,)


def _problem(kind):
    """(orig_level, base_level, base_state, music_mask, frame_starts, kwargs)."""
    rng = np.random.default_rng(11)
    F = 150
    k = np.arange(F)
    state = np.where((k // 15) % 2 == 1, 2, 1).astype(np.int32)
    mask = rng.random(F) < 0.8
    mask[0] = True
    kw = {}
    if kind == "two_valued":
        # every T between the two values (and every hyst that keeps both
        # thresholds between them) fits alike: the first in loop order wins
        orig = np.where(state == 2, -20.0, -50.0).astype(np.float32)
    elif kind == "noisy":
        orig = (np.where(state == 2, -28.0, -36.0) + rng.normal(0, 4.0, F)).astype(np.float32)
        kw = dict(hyst_list=(0, 0.3, 1), delay_list_ms=(0, 30, 100), T_step_db=0.5,
                  gain_search_pm_db=1.0)
    elif kind in ("ten_c2", "nine_c2"):
        # the < 10 rule counts fitted target frames, so it skips every gain or none
        n2 = 10 if kind == "ten_c2" else 9
        state = np.ones(F, np.int32)
        mask = np.ones(F, bool)
        mask[3::7] = False
        fit = np.flatnonzero(mask)
        state[fit[40:40 + n2]] = 2
        orig = (np.where(state == 2, -25.0, -40.0) + rng.normal(0, 2.0, F)).astype(np.float32)
    else:
        raise ValueError(kind)
    base = (orig + np.float32(2.25) + rng.normal(0, 0.1, F).astype(np.float32)).astype(np.float32)
    return orig, base, state, mask, (k * 2048).astype(np.int64), kw


@pytest.mark.parametrize("kind", ["two_valued", "noisy", "ten_c2", "nine_c2"])
def test_search_grid_fitting_problems(kind):
    _, cal = _cal()
    orig, base, state, mask, fs, kw = _problem(kind)
    want = R.search(orig, base, state, mask, fs, SR, **kw)
    got = cal.search_grid(orig, state, mask, fs, SR, base_level=base, **kw)
    assert got == want, (got, want)
    if kind == "nine_c2":
        assert got[0] is None and got[2] == 0
    else:
        assert got[0] is not None and got[2] > 0
    if kind == "two_valued":
        best = got[0]
        # the winner is the first of many that tie
        rows, fs_fit, s_fit, cands, meta, _ = R.search_table(orig, base, state, mask, fs, SR)
        cnt = R.grid_counts(rows, fs_fit, s_fit, cands)
        ties = np.flatnonzero((cnt == [int(round(best["mismatch"] * len(s_fit))),
                                       best["switches"]]).all(axis=1))
        assert len(ties) > 100
        assert meta[ties[0]][1:5] == (best["T"], best["hyst"], best["up_ms"], best["gain_db"])


# ---------------------------------------------------------------------------
# band energies
# ---------------------------------------------------------------------------

BAND_SIZES = [(16, 5), (100, 37), (3000, 750), (4096, 2048), (8191, 4000), (16384, 8192)]
BAND_FRAMES = (1, 2, 5)


def _band_signal(n_fft, hop, F):
    """Stereo white noise giving F frames (and a few samples more); the block
    of hop samples that frame f begins with, and for the last frame everything
    after it, is scaled by 1 + f, so two frames mixed up differ by O(1)."""
    n = n_fft + (F - 1) * hop + min(hop - 1, 3)
    x = white(4000 + n_fft + F, n, 2, amp=0.1)
    x *= (1.0 + np.minimum(np.arange(n) // hop, F - 1)).astype(np.float32)[:, None]
    assert 1 + (n - n_fft) // hop == F
    return x


def _band_power(x, n_fft, hop):
    """(P64, P32) [F][n_fft/2+1]: re^2 + im^2 of rfft(hanning * power_mono(frame)) in
    float64 and in float32 numpy."""
    from scipy import fft as sfft
    w32 = np.hanning(n_fft).astype(np.float32)
    x64 = x.astype(np.float64)
    m64 = np.sqrt(0.5 * (x64[:, 0] * x64[:, 0] + x64[:, 1] * x64[:, 1]) + EPS)
    m32 = np.sqrt(np.float32(0.5) * (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + np.float32(EPS))
    assert m32.dtype == np.float32
    F = 1 + (len(x) - n_fft) // hop
    P64 = np.empty((F, n_fft // 2 + 1), np.float64)
    P32 = np.empty((F, n_fft // 2 + 1), np.float32)
    for f in range(F):
        X = np.fft.rfft(m64[f * hop:f * hop + n_fft] * w32.astype(np.float64))
        P64[f] = X.real * X.real + X.imag * X.imag
        Y = sfft.rfft(m32[f * hop:f * hop + n_fft] * w32)
        assert Y.dtype == np.complex64
        P32[f] = Y.real * Y.real + Y.imag * Y.imag
    return P64, P32


def _sums(P, bands, dt):
    out = np.zeros((len(P), 2), dt)
    for f in range(len(P)):
        for b, (k0, k1) in enumerate(bands):
            out[f, b] = np.sum(P[f, k0:k1], dtype=dt)
    return out


def _hz_bins(n_fft, band):
    freqs = np.fft.rfftfreq(n_fft, 1 / SR)
    idx = np.flatnonzero((freqs >= band[0]) & (freqs < band[1]))
    assert len(idx) == 0 or np.array_equal(idx, np.arange(idx[0], idx[-1] + 1))
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def _bins_hz(n_fft, bins):
    """A band in Hz holding exactly bins [k0, k1) (none: a band between two bins)."""
    df = SR / n_fft
    k0, k1 = bins
    return ((k0 - 0.5) * df, (k1 - 0.5) * df) if k1 > k0 else (0.25 * df, 0.3 * df)


def _band_sets(n_fft, overlap=True):
    """name -> ((lo0, lo1), (hi0, hi1)) in bins."""
    nb = n_fft // 2 + 1
    m = nb // 2
    sets = {
        "defaults": (_hz_bins(n_fft, (200, 1000)), _hz_bins(n_fft, (2000, 8000))),
        "dc | nyquist": ((0, 1), (nb - 1, nb)),
        "all | empty": ((0, nb), (m, m)),
        "empty | one bin": ((nb, nb), (m, m + 1)),
        "touching": ((1, m), (m, nb - 1)),
        "lo above hi": ((m + 1, nb), (0, m)),
    }
    if overlap:
        sets["overlapping"] = ((1, 2 * nb // 3), (nb // 3, nb))
        sets["nested"] = ((0, nb), (2, nb - 2))
        sets["identical"] = ((1, m), (1, m))
    return sets


def _band_energy(torch, x, n_fft, hop, bands):
    from tomatis_audio_processor_amd import dsp
    lib = _L()
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    F = 1 + (len(x) - n_fft) // hop
    out = torch.full((F + 1, 2), -3.0, dtype=torch.float32, device="cuda")
    (lo0, lo1), (hi0, hi1) = bands
    rc = lib.lib().tomatis_an_band_energy(lib.ptr(xd), len(x), n_fft, hop, lo0, lo1, hi0, hi1,
                                          lib.ptr(win), lib.ptr(out), lib.stream_handle())
    assert rc == 0, (rc, bands)
    o = out.cpu().numpy()
    assert np.all(o[F] == -3.0), "wrote past the last frame"
    return o[:F]


def _rel_errors(got, E64, E32, bands):
    """(e, e32) over the frames and the non-empty bands; empty bands are 0."""
    e = e32 = 0.0
    for b, (k0, k1) in enumerate(bands):
        if k1 <= k0:
            assert np.all(got[:, b] == 0.0), ("empty band", b, got[:, b])
            continue
        assert np.all(E64[:, b] > 0.0)
        e = max(e, float(np.max(np.abs(got[:, b] - E64[:, b]) / E64[:, b])))
        e32 = max(e32, float(np.max(np.abs(E32[:, b].astype(np.float64) - E64[:, b]) / E64[:, b])))
    return e, e32


def _tilt64(E64):
    return 10 * np.log10((E64[:, 1] + EPS) / (E64[:, 0] + EPS) + EPS)


def _tilt_tol(tilt, B):
    """A tilt from band sums each within a relative B of the float64 sums: the
    two errors and the float32 roundings of E + EPS (2^-24 each) move the ratio
    by at most their sum, to first order, so the tilt by 10 / ln 10 times that
    (1 % for the higher orders); the float32 result adds half an ulp."""
    return 10 / np.log(10) * 1.01 * (2 * B + 2.0 ** -23) + np.abs(tilt) * 2.0 ** -23


@pytest.mark.parametrize("F", BAND_FRAMES)
@pytest.mark.parametrize("n_fft,hop", BAND_SIZES)
def test_band_energies(n_fft, hop, F):
    torch, cal = _cal()
    x = _band_signal(n_fft, hop, F)
    P64, P32 = _band_power(x, n_fft, hop)
    path = "band pow2" if n_fft & (n_fft - 1) == 0 else "band Bluestein"
    failed = []
    for name, bands in _band_sets(n_fft).items():
        E64, E32 = _sums(P64, bands, np.float64), _sums(P32, bands, np.float32)
        got = _band_energy(torch, x, n_fft, hop, bands)
        assert got.shape == E64.shape
        e, e32 = _rel_errors(got, E64, E32, bands)
        print(f"RATIO [{path}] {n_fft}/{hop} F {F} {name}: e {e:.3e} e32 {e32:.3e} "
              f"ratio {e / max(e32, FLOOR):.2f}")
        B = bound(e32, FACTOR)
        if not e <= B:
            failed.append((name, e, e32))
        # the same bands in Hz through band_tilts
        tilts = cal.band_tilts(x, SR, n_fft, hop, _bins_hz(n_fft, bands[0]),
                               _bins_hz(n_fft, bands[1]))
        want = _tilt64(E64)
        assert tilts.dtype == np.float32 and tilts.shape == want.shape
        d = np.abs(tilts - want)
        print(f"TILT [{path}] {n_fft}/{hop} F {F} {name}: max |d| {d.max():.3e} dB "
              f"tol {_tilt_tol(want, B).min():.3e}")
        if not np.all(d <= _tilt_tol(want, B)):
            failed.append((name, "tilt", float(d.max())))
    assert not failed, (n_fft, hop, F, failed)


def test_band_energy_argument_errors():
    torch, _ = _cal()
    lib = _L()
    from tomatis_audio_processor_amd import dsp
    L, ptr, hs = lib.lib(), lib.ptr, lib.stream_handle()
    n_fft, hop, nb = 64, 16, 33
    x = torch.zeros((n_fft + hop, 2), dtype=torch.float32, device="cuda")
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    out = torch.full((2, 2), -3.0, dtype=torch.float32, device="cuda")
    null = C.c_void_p(0)
    ok = dict(x=ptr(x), n=n_fft + hop, n_fft=n_fft, hop=hop, lo0=2, lo1=5, hi0=8, hi1=20,
              win=ptr(win), out=ptr(out))
    for change in (dict(x=null), dict(win=null), dict(out=null), dict(hop=0), dict(n_fft=0),
                   dict(lo0=-1), dict(lo1=1), dict(lo1=nb + 1), dict(hi0=-1), dict(hi1=7),
                   dict(hi1=nb + 1)):
        a = dict(ok, **change)
        rc = L.tomatis_an_band_energy(a["x"], a["n"], a["n_fft"], a["hop"], a["lo0"], a["lo1"],
                                      a["hi0"], a["hi1"], a["win"], a["out"], hs)
        assert rc == lib.E_ARG, change
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


def test_calibrate_with_overlapping_tilt_bands(tmp_path):
    """--tilt_lo 200 3000 --tilt_hi 2000 8000, which the reference takes: the
    command runs and its tilts are the float64 formula's."""
    torch, cal = _cal()
    from tests.golden.calib_case import CASE, make_inputs
    from tomatis_audio_processor_amd import audio_io
    xo, xb = make_inputs()
    po, pb = str(tmp_path / "orig.wav"), str(tmp_path / "base.wav")
    audio_io.write(po, xo, CASE["sr"], "WAV", "FLOAT")
    audio_io.write(pb, xb, CASE["sr"], "WAV", "FLOAT")
    n_fft, hop, lo, hi = CASE["n_fft"], CASE["hop"], (200, 3000), (2000, 8000)
    out, aux = cal.calibrate(po, pb, max_minutes=0.25, tilt_lo=lo, tilt_hi=hi,
                             log=lambda *a: None)
    d = out["delay_samples_orig_minus_base"]
    assert d == int(fixture()["delay"])
    bs = max(0, -d)
    avail = min(len(xb) - bs, len(xo) - max(0, d), int(0.25 * 60 * CASE["sr"]))
    seg = xb[bs:bs + avail]
    bands = (_hz_bins(n_fft, lo), _hz_bins(n_fft, hi))
    assert bands[0][1] > bands[1][0] and bands[1][1] > bands[0][0], "the bands overlap"
    P64, P32 = _band_power(seg, n_fft, hop)
    E64, E32 = _sums(P64, bands, np.float64), _sums(P32, bands, np.float32)
    e32 = float(np.max(np.abs(E32.astype(np.float64) - E64) / E64))
    want = _tilt64(E64)
    assert aux["tilts"].shape == want.shape
    dmax = np.abs(aux["tilts"] - want)
    tol = _tilt_tol(want, bound(e32, FACTOR))
    print(f"TILT [calibrate] overlapping bands: max |d| {dmax.max():.3e} dB e32 {e32:.3e} "
          f"tol {tol.min():.3e}")
    assert np.all(dmax <= tol)
    assert aux["best"] is not None
