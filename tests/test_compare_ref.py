"""CPU: the numpy / scipy restatement of compare_audio (tests/compare_ref.py)
reproduces the reference's goldens, the mean-first envelope formula the device
implements is resample_poly's, and the host logic of
tomatis_audio_processor_amd.compare_audio (no device needed)."""
import functools
import inspect

import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import compare_ref as cr
from tests.golden.compare_cases import (DELAY_CASES_FULL, ERROR_CASES, MAIN_CASES, MIN_MARGIN, SR,
                                        make_inputs)
from tests.golden_util import sha
from tests.stft_ref import white


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(c for c in DELAY_CASES_FULL + MAIN_CASES + ERROR_CASES if c["name"] == name)
    return make_inputs(c)


# ---------------------------------------------------------------------------
# the restatement equals the goldens
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c["name"] for c in DELAY_CASES_FULL])
def test_restated_delay_equals_golden(name):
    fx = cr.fixture(name)
    base, cand = _inputs(name)
    assert [sha(base), sha(cand)] == list(fx["in_sha"])
    assert float(fx["margin64"]) >= MIN_MARGIN
    st = cr.delay_estimate(base, cand, SR, 2000)
    assert (st["delay"], st["k"], st["nb"]) == (int(fx["delay"]), int(fx["k"]), int(fx["nb"]))


def test_short_pairs_margin_in_float64():
    """The stored margin is the float64 correlation's (np.correlate)."""
    for name in ("compare_short_base", "compare_short_target"):
        fx = cr.fixture(name)
        base, cand = _inputs(name)
        st = cr.delay_estimate(base, cand, SR, 2000, np.float64)
        assert st["k"] == int(fx["k"])
        assert cr.margin(st["corr"]) == pytest.approx(float(fx["margin64"]), rel=1e-9)


@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_restated_main_equals_golden(name):
    c = next(c for c in MAIN_CASES if c["name"] == name)
    fx = cr.fixture(name)
    base, cand = _inputs(name)
    n = cr.main_numbers(base, cand, SR, c["n_fft"], c["hop"])
    assert cr.report(n) == str(fx["stdout"])
    assert n["delay"] == int(fx["delay"])
    for key in ("b_mag", "c_mag", "c_mag2", "diff_db"):
        assert n[key].dtype == np.float32
        assert np.array_equal(n[key], fx[key]), key
    assert np.array_equal(n["freqs"], fx["freqs"])
    assert (n["gain_db"], n["gain_lin"], n["snr_db"]) == (float(fx["gain_db"]),
                                                          float(fx["gain_lin"]),
                                                          float(fx["snr_db"]))
    # float64 throughout moves the numbers by float32 rounding only
    n64 = cr.main_numbers(base, cand, SR, c["n_fft"], c["hop"], np.float64, delay=n["delay"])
    assert abs(n64["gain_db"] - n["gain_db"]) < 1e-4 and abs(n64["snr_db"] - n["snr_db"]) < 1e-4


def test_restated_error_equals_golden():
    c = ERROR_CASES[0]
    base, cand = _inputs(c["name"])
    with pytest.raises(ValueError) as ei:
        cr.main_numbers(base, cand, SR, c["n_fft"], c["hop"])
    assert str(ei.value) == str(cr.fixture(c["name"])["error"])


# ---------------------------------------------------------------------------
# the mean-first envelope formula
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("down", [24, 6])
@pytest.mark.parametrize("n", [1, 23, 24, 25, 481, 4801])
def test_mean_first_formula_is_resample_poly(n, down):
    x = white(9000 + n + down, n, 2)
    y, mean = cr.envelope_mean_first(x, 48000, 48000 // down, np.float64)
    d = cr.envelope_mean_first_direct(x, down)
    assert y.shape == d.shape == (-(-n // down),)
    assert mean == cr.power_mono(x, np.float64).mean()
    # resample_poly designs its taps in float64 for float64 input; the device's are that
    # filter rounded to float32 (what resample_poly uses on the reference's float32 input):
    # each tap moves by at most 2^-24 of itself
    from scipy.signal import firwin
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0))
    dev = np.max(np.abs(cr.power_mono(x, np.float64) - mean))
    assert np.max(np.abs(y - d)) <= 2.0 ** -24 * np.sum(np.abs(h)) * dev + 1e-15


def test_mean_first_edges_are_zero_not_minus_mean():
    """e - mu is zero outside the signal: extending e by zeros before the mean
    is removed (-mu outside) is another signal at the edges, and removing the
    mean after the decimation (layer2_analyze_eq's order) another one."""
    down = 24
    x = white(9100, 4801, 2)
    e = cr.power_mono(x, np.float64)
    d = cr.envelope_mean_first_direct(x, down)
    pad = 10 * down
    wrong = resample_poly(np.concatenate([np.zeros(pad), e, np.zeros(pad)]) - e.mean(), 1, down)
    wrong = wrong[pad // down:pad // down + len(d)]
    assert abs(wrong[0] - d[0]) > 1e-2 and abs(wrong[-1] - d[-1]) > 1e-2
    # the interior agrees (float64 taps against float32-rounded ones: 2^-24 per tap)
    assert np.max(np.abs(wrong[20:-20] - d[20:-20])) < 1e-7
    last = resample_poly(e, 1, down)
    last = last - last.mean()
    assert np.max(np.abs(last - d)) > 1e-2


# ---------------------------------------------------------------------------
# host logic of the module
# ---------------------------------------------------------------------------

def test_align_pair_offsets():
    from tomatis_audio_processor_amd import compare_audio as ca
    b, c = np.arange(20).reshape(10, 2), np.arange(100, 124).reshape(12, 2)
    for delay in (3, -4, 0, 11, -10, 12):
        wb, wc = cr.align_pair(b, c, delay)
        gb, gc = ca.align_pair(b, c, delay)
        assert np.array_equal(gb, wb) and np.array_equal(gc, wc)
        b0, c0, n = ca.align_offsets(len(b), len(c), delay)
        assert n == len(wb) == len(wc)
        assert np.array_equal(b[b0:b0 + n], wb) and np.array_equal(c[c0:c0 + n], wc)
    assert ca.align_offsets(10, 12, 3) == (0, 3, 9)
    assert ca.align_offsets(10, 12, -4) == (4, 0, 6)
    assert ca.align_offsets(10, 12, 0) == (0, 0, 10)
    assert ca.align_offsets(10, 12, 12)[2] == 0 and ca.align_offsets(10, 12, -30)[2] == 0


def test_band_energy_rms_db_power_mono():
    from tomatis_audio_processor_amd import compare_audio as ca
    freqs = np.fft.rfftfreq(64, 1 / 48000)
    mag = np.linspace(0.1, 2.0, 33).astype(np.float32)
    assert ca.band_energy(mag, freqs, 300, 3000) == cr.band_energy(mag, freqs, 300, 3000)
    m = (freqs >= 3000) & (freqs < 8000)
    assert ca.band_energy(mag, freqs, 3000, 8000) == float(np.mean(mag[m] ** 2) + 1e-12)
    x = white(9200, 100, 2)
    pm = ca.power_mono(x)
    assert pm.dtype == np.float32 and np.array_equal(pm, cr.power_mono(x))
    assert ca.rms_db(pm) == cr.rms_db(pm)
    assert ca._rms_db_of_mean(float(np.mean(pm.astype(np.float64) ** 2))) == pytest.approx(
        float(cr.rms_db(pm)), abs=1e-5)


def test_cli_and_main_defaults():
    from tomatis_audio_processor_amd import compare_audio as ca
    a = ca.build_parser().parse_args(["b.flac", "c.flac"])
    assert (a.base, a.cand) == ("b.flac", "c.flac") and set(vars(a)) == {"base", "cand"}
    with pytest.raises(SystemExit):
        ca.build_parser().parse_args(["only_one"])
    sig = inspect.signature(ca.main)
    assert list(sig.parameters) == ["base_path", "cand_path", "sr", "n_fft", "hop", "out_csv"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [48000, 4096, 2048,
                                                                       "diff_spectrum.csv"]
    for name in ("power_mono", "stft_mag_avg", "band_energy", "find_delay_by_corr", "align_pair",
                 "rms_db", "main", "compare"):
        assert callable(getattr(ca, name))


def test_asserts_need_no_device(tmp_path):
    from tomatis_audio_processor_amd import audio_io, compare_audio as ca
    x = white(9300, 4800, 2)
    with pytest.raises(AssertionError):
        ca.compare(x[:, :1], x, log=lambda s: None)          # not stereo
    with pytest.raises(AssertionError):
        ca.compare(x, np.concatenate([x, x], axis=1), log=lambda s: None)
    p = str(tmp_path / "a44.wav")
    audio_io.write(p, x, 44100, "WAV", "FLOAT")
    with pytest.raises(AssertionError):
        ca.main(p, p, out_csv=str(tmp_path / "no.csv"))       # wrong sample rate
    assert not (tmp_path / "no.csv").exists()


def test_host_bodies_equal_golden():
    """The scipy body behind the ratios the decimator leaves out, and
    find_delay_by_corr on the reference's own 1-D power-mono arguments."""
    from tomatis_audio_processor_amd import align, compare_audio as ca
    name = "compare_p1234"
    base, cand = _inputs(name)
    want = int(cr.fixture(name)["delay"])
    assert align._find_delay_full_host(base, cand, SR, 2000) == want
    assert ca.find_delay_by_corr(ca.power_mono(base), ca.power_mono(cand), SR) == want
    assert not align.device_ratio(SR, 1800)
    assert align.find_delay_full(base, cand, sr=SR, ds_sr=1800) == \
        cr.delay_estimate(base, cand, SR, 1800)["delay"]
    assert align._delay_full(24050, 24000, SR, 2000) == 1224


def test_new_entry_points_are_bound():
    from tomatis_audio_processor_amd import _lib
    for name in ("tomatis_align_envelope_mean_first", "tomatis_fft_pow2_work_bytes",
                 "tomatis_fft_pow2", "tomatis_align_xcorr_full_work_bytes",
                 "tomatis_align_xcorr_full", "tomatis_compare_residual"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 11
    import re, os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "tomatis_hip.h")).read()
    defs = dict(re.findall(r"#define (TOMATIS_[A-Z0-9_]+) \(?(-?\d+)u?\)?", src))
    assert int(defs["TOMATIS_RESIDUAL_DOUBLES"]) == _lib.RESIDUAL_DOUBLES
    assert (int(defs["TOMATIS_FFT_MIN_LOG2"]), int(defs["TOMATIS_FFT_MAX_LOG2"])) == \
        (_lib.FFT_MIN_LOG2, _lib.FFT_MAX_LOG2)
