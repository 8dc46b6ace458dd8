"""CPU: the numpy / scipy restatement of compare_to_baseline (tests/baseline_ref.py)
reproduces the reference's goldens (tools/make_baseline_goldens.py), the new
entry points are declared, bound and exported under ABI 11, and the host logic
of tomatis_audio_processor_amd.compare_to_baseline (no device needed)."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests import baseline_ref as br
from tests.golden.baseline_cases import (BASELINE_FILE, ERROR_CASES, MAIN_CASES, MIN_MARGIN, OUTDIR,
                                         SR, make_inputs)
from tests.golden_util import sha
from tests.stft_ref import white

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_KEYS = [k for k, _, _ in br.BANDS]
NEW = ("tomatis_an_spectrum_mean", "tomatis_an_spectrum_mean_work_doubles",
       "tomatis_cmp_mono_sums")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return make_inputs(next(c for c in MAIN_CASES + ERROR_CASES if c["name"] == name))


@functools.lru_cache(maxsize=None)
def _run(name):
    c = next(c for c in MAIN_CASES if c["name"] == name)
    base, cands = _inputs(name)
    return br.run(base, cands, SR, c["n_fft"], c["hop"], c["max_minutes"])


# ---------------------------------------------------------------------------
# the restatement equals the goldens
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_restated_run_equals_golden(name):
    c = next(c for c in MAIN_CASES if c["name"] == name)
    fx = br.fixture(name)
    base, cands = _inputs(name)
    assert [sha(base)] + [sha(x) for x in cands] == list(fx["in_sha"])
    rs = _run(name)
    assert len(rs) == int(fx["n_cands"]) == len(c["cands"])
    files = [k["file"] for k in c["cands"]]
    assert br.summary_text(BASELINE_FILE, files, rs, SR, c["max_minutes"]) == str(fx["summary"])
    assert br.stdout_text(OUTDIR, files) == str(fx["stdout"])
    assert str(fx["header"]) == br.CSV_HEADER
    for i, r in enumerate(rs):
        assert float(fx[f"margin64_{i}"]) >= MIN_MARGIN
        assert r["delay"] == int(fx[f"delay_{i}"])
        cols = br.csv_columns(r)
        assert cols.dtype == np.float32 and np.array_equal(cols, fx[f"cols_{i}"])
        assert np.array_equal(cols[:, 0], np.fft.rfftfreq(c["n_fft"], 1 / SR).astype(np.float32))
        got = (r["gain_db"], r["anchor"], r["snr"], r["music_err"], r["noise_delta"])
        assert got == tuple(float(fx[f"{k}_{i}"]) for k in ("gain_db", "anchor", "snr", "music_err",
                                                             "noise_delta"))
        assert [r["stats"][k] for k in BAND_KEYS] == list(fx[f"stats_{i}"])


def test_cap_bites_and_single_lag():
    """--max_minutes 0.5 cuts the 40 s overlaps to 30 s; the 12 s pair's valid
    correlation has one lag, so its delay is 0 and not the shift."""
    c = MAIN_CASES[0]
    base, cands = _inputs(c["name"])
    for cand, r in zip(cands, _run(c["name"])):
        b, _ = br.overlap(base, cand, r["delay"], SR, c["max_minutes"])
        assert len(b) == int(0.5 * 60 * SR) < min(len(base), len(cand)) - abs(r["delay"])
    # within the estimate's resolution (the decimation, 24) of the shifts
    assert [abs(r["delay"] - k["shift"]) <= 24 for r, k in zip(_run(c["name"]), c["cands"])] == \
        [True, True]
    c = MAIN_CASES[2]
    base, cands = _inputs(c["name"])
    st = br.find_delay(cands[0], base, SR)
    assert len(st["corr"]) == 1 and st["delay"] == 0 != c["cands"][0]["shift"]
    assert float(br.fixture(c["name"])["margin64_0"]) == np.inf


def test_float64_run_moves_by_float32_rounding_only():
    name = "baseline_m3210_1024"
    c = next(c for c in MAIN_CASES if c["name"] == name)
    fx = br.fixture(name)
    base, cands = _inputs(name)
    r, = _run(name)
    q, = br.run(base, cands, SR, c["n_fft"], c["hop"], c["max_minutes"], np.float64, [r["delay"]])
    for k, i in (("Sb", 0), ("Sc", 1)):
        e32 = float(np.max(np.abs(r[k].astype(np.float32).astype(np.float64) - q[k])))
        assert e32 == float(fx["e32_0"][i]) < 1e-5
        assert float(np.max(np.abs(q[k]))) == float(fx["smax_0"][i])
    assert abs(q["gain_db"] - r["gain_db"]) < 1e-4 and abs(q["snr"] - r["snr"]) < 1e-4
    assert br.db_bound(0.0, 100.0) == 8 * 2.0 ** -17 and br.db_bound(1e-3, 100.0) == 8e-3


@pytest.mark.parametrize("name", [c["name"] for c in ERROR_CASES[:2]])
def test_restated_error_equals_golden(name):
    c = next(c for c in ERROR_CASES if c["name"] == name)
    base, cands = _inputs(name)
    with pytest.raises(ValueError) as ei:
        br.run(base, cands, SR, c["n_fft"], c["hop"], c["max_minutes"])
    assert str(ei.value) == str(br.fixture(name)["error"])


# ---------------------------------------------------------------------------
# header, binding, exports
# ---------------------------------------------------------------------------

def test_new_entry_points_are_declared_and_bound():
    from tomatis_audio_processor_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomatis_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(tomatis_[a-z0-9_]+)\s*\(", code))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGS
    assert set(_lib.EXPORTS) == declared
    assert src.count("compare_to_baseline.py:105-122") >= 1
    defs = dict(re.findall(r"#define (TOMATIS_[A-Z0-9_]+) \(?(-?\d+)u?\)?", src))
    assert int(defs["TOMATIS_ABI_VERSION"]) == _lib.ABI_VERSION == 11
    assert int(defs["TOMATIS_MONO_SUMS_DOUBLES"]) == _lib.MONO_SUMS_DOUBLES == \
        3 + 3 * (int(defs["TOMATIS_ALIGN_MEAN_DOUBLES"]) - 1)
    assert len(_lib._SIGS["tomatis_an_spectrum_mean"][1]) == 11
    assert len(_lib._SIGS["tomatis_cmp_mono_sums"][1]) == 6


def test_library_exports_the_new_symbols():
    import ctypes
    from tomatis_audio_processor_amd import _lib
    path = _lib.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() first")
    h = ctypes.CDLL(path)
    assert all(hasattr(h, n) for n in NEW)
    assert h.tomatis_abi_version() == 11
    wd = h.tomatis_an_spectrum_mean_work_doubles
    wd.restype, wd.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]
    # one row of n_bins doubles per slab of 8 frame pairs; nothing outside the range
    assert [wd(F, 2049) // 2049 for F in (1, 2, 16, 17, 18, 11249)] == [1, 1, 1, 2, 2, 704]
    assert wd(0, 2049) == wd(5, 0) == wd(1 << 31, 9) == 0


# ---------------------------------------------------------------------------
# host logic of the module
# ---------------------------------------------------------------------------

def test_host_functions_equal_the_restatement():
    from tomatis_audio_processor_amd import compare_to_baseline as cb
    x = white(9400, 300, 2)
    pm = cb.power_mono(x)
    assert pm.dtype == np.float32 and np.array_equal(pm, br.power_mono(x))
    assert np.array_equal(cb.power_mono(x[:, :1]), np.abs(x[:, 0]))
    with pytest.raises(ValueError, match=r"audio must be \[N, C\]"):
        cb.power_mono(x[:, 0])
    r = np.sqrt(np.mean(pm * pm) + 1e-12)
    assert cb.rms_dbfs_from_mono(pm) == float(20.0 * np.log10(r + 1e-12))
    d = np.cumsum(white(9401, 200, 1)[:, 0]).astype(np.float32)
    s = cb.smooth_1d(d)
    assert s.dtype == np.float32 and s.shape == d.shape and np.array_equal(s, br.smooth_1d(d))
    assert np.array_equal(cb.smooth_1d(d, 1), d) and cb.smooth_1d(d, 1) is not d
    freqs = np.fft.rfftfreq(398, 1 / 48000).astype(np.float32)
    for lo, hi in ((300.0, 3000.0), (80, 200), (8000, 16000)):
        assert cb.band_mean(freqs, d, lo, hi) == br.band_mean(freqs, d, lo, hi)
    assert np.isnan(cb.band_mean(freqs, d, 1.0, 2.0))
    assert cb.BANDS == br.BANDS and cb.CSV_HEADER == br.CSV_HEADER


def test_cli_and_signatures():
    from tomatis_audio_processor_amd import compare_to_baseline as cb
    a = cb.build_parser().parse_args(["--baseline", "b.flac", "--candidates", "c1.flac", "c2.flac",
                                      "--outdir", "o"])
    assert vars(a) == dict(baseline="b.flac", candidates=["c1.flac", "c2.flac"], outdir="o",
                           sr=48000, n_fft=4096, hop=2048, max_minutes=8.0)
    with pytest.raises(SystemExit):
        cb.build_parser().parse_args(["--baseline", "b.flac", "--outdir", "o"])

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(cb.find_delay_by_corr) == [("cand", E), ("base", E), ("sr", 48000),
                                          ("ds_sr", 2000), ("chunk_sec", 25)]
    assert sig(cb.get_aligned_overlap) == [("base", E), ("cand", E), ("sr", 48000),
                                           ("max_minutes", None)]
    assert sig(cb.compute_metrics)[2:] == [("sr", 48000), ("n_fft", 4096), ("hop", 2048)]
    assert sig(cb.frame_rms_dbfs)[1:] == [("sr", E), ("win_ms", 50), ("hop_ms", 25)]
    assert sig(cb.compare_many)[:7] == [("baseline", E), ("candidates", E), ("outdir", E),
                                        ("sr", 48000), ("n_fft", 4096), ("hop", 2048),
                                        ("max_minutes", 8.0)]


def test_rate_and_mono_errors_need_no_device(tmp_path):
    from tomatis_audio_processor_amd import audio_io, compare_to_baseline as cb
    c = ERROR_CASES[2]
    fx = br.fixture(c["name"])
    base, (cand,) = _inputs(c["name"])
    pb, pc = str(tmp_path / BASELINE_FILE), str(tmp_path / c["cands"][0]["file"])
    audio_io.write(pb, base, SR, "WAV", "FLOAT")
    audio_io.write(pc, cand, c["cands"][0]["sr"], "WAV", "FLOAT")
    out = tmp_path / "out"
    with pytest.raises(ValueError) as ei:
        cb.main(["--baseline", pb, "--candidates", pc, "--outdir", str(out)])
    assert str(ei.value) == str(fx["error"]) == "sample rate mismatch"
    with pytest.raises(ValueError) as ei:
        cb.get_aligned_overlap(pb, pc)
    assert str(ei.value) == str(fx["error"])
    with pytest.raises(ValueError) as ei:
        cb.find_delay_by_corr(pc, pb)
    assert str(ei.value) == str(fx["error_find_delay"])
    assert not (out / "summary.txt").exists()
    # the one narrowing: a mono file says so
    pm = str(tmp_path / "mono.wav")
    audio_io.write(pm, base[:, :1], SR, "WAV", "FLOAT")
    with pytest.raises(ValueError, match="stereo only"):
        cb.find_delay_by_corr(pm, pb)
    with pytest.raises(ValueError, match="stereo only"):
        cb.compare_many(pb, [pm], str(out))
    with pytest.raises(ValueError, match="segment too short"):
        cb.avg_spectrum_db(np.zeros((100, 2), np.float32), SR, 4096, 2048)
