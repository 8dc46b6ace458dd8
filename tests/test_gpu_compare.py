"""GPU: compare_audio on the device: the power-of-two FFT
in global memory and the full correlation built on it (tm_fftcorr.hip), the
mean-first envelope and the residual means (tm_align.hip), ``align.
find_delay_full`` and ``compare_audio.compare`` / ``main`` against the
reference's goldens (tools/make_compare_goldens.py).

Transforms, correlation and envelope are judged like the other transforms
(tests/test_gpu_spectral_fidelity.py, tests/align_ref.py): with the float64
numpy statement y64 of the operation and scipy's own float32 result y32 of it,

    e = max |y - y64| / max |y64|  <=  8 * max(e32, 2^-23),  e32 = the same of y32.

Delays are compared as integers after the stored float64 margin of the
correlation's top, (top - runner-up) / top, is shown to be >= 1e-3.

Largest measured e / max(e32, 2^-23) on the MI355X: FFT 1.13 (inverse, 2^14;
1.87 for ifft(fft(x)) at 2^14), full correlation 0.99 (nc = nb = 9; 0.55 at
24000 x 24000), mean-first envelope 1.47 (24 samples, down 24; 0.43 at 240017).
"""
import contextlib
import functools
import io
import os
import re
import tempfile

import numpy as np
import pytest
import scipy.fft
from scipy.signal import fftconvolve

from tests import compare_ref as cr
from tests.golden.compare_cases import (DELAY_CASES_FULL, ERROR_CASES, MAIN_CASES, MIN_MARGIN, SR,
                                        make_inputs)
from tests.stft_ref import white

pytestmark = pytest.mark.gpu

MAG_RTOL = 2e-5   # tests/test_gpu_analysis.py: a mean spectrum, relative to its maximum
DB_ATOL = 2e-3    # tests/test_gpu_analysis.py: dB


@pytest.fixture(scope="module")
def al():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, align
    _lib.lib()
    return align


def _rel(y, y64):
    return float(np.max(np.abs(np.asarray(y).astype(y64.dtype) - y64)) / np.max(np.abs(y64)))


# ---------------------------------------------------------------------------
# the FFT.  Sizes mirror tm_fftcorr.hip: kMinLog = 4 (and 5: the radix-2 first
# stage), kRowLog = 13 (the largest single-workgroup transform), 14 (the first
# six-step one, N1 = N2 = 128), 15 (N1 = 256 != N2 = 128: two tables), 2^20.
# There is no further switch: the six-step split holds up to kMaxLog = 25.
# ---------------------------------------------------------------------------
FFT_LOGS = [4, 5, 13, 14, 15, 20]


@functools.lru_cache(maxsize=None)
def _fft_case(p):
    """-> (x complex64, X64, e32 of scipy.fft's float32 transform)."""
    rng = np.random.default_rng(5000 + p)
    n = 1 << p
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    X64 = np.fft.fft(x.astype(np.complex128))
    X32 = scipy.fft.fft(x)
    assert X32.dtype == np.complex64
    return x, X64, _rel(X32, X64)


@pytest.mark.parametrize("p", FFT_LOGS)
def test_fft_forward_inverse_round_trip(al, p):
    x, X64, e32 = _fft_case(p)
    X = al.fft_pow2(x)
    got = X.cpu().numpy()
    assert got.dtype == np.complex64 and got.shape == x.shape
    e = _rel(got, X64)
    # the inverse on its own: of the float64 spectrum rounded to float32
    Xr = X64.astype(np.complex64)
    x64 = np.fft.ifft(Xr.astype(np.complex128))
    ei32 = _rel(scipy.fft.ifft(Xr), x64)
    ei = _rel(al.fft_pow2(Xr, inverse=True).cpu().numpy(), x64)
    # ifft(fft(x)) on the device
    back = al.fft_pow2(X, inverse=True).cpu().numpy()
    er = _rel(back, x.astype(np.complex128))
    fl = cr.FLOOR
    print(f"RATIO [fft] 2^{p}: forward {e / max(e32, fl):.2f} inverse {ei / max(ei32, fl):.2f} "
          f"round trip {er / max(e32, fl):.2f} (e32 {e32:.3e})")
    assert e <= cr.bound(e32), (p, e, e32)
    assert ei <= cr.bound(ei32), (p, ei, ei32)
    assert er <= cr.bound(e32), (p, er, e32)
    again = al.fft_pow2(x).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "run-to-run"


def test_fft_largest_length_impulses(al):
    """2^25 (kMaxLog) once: a handful of impulses, sampled bins against the
    closed form X[k] = sum_j a_j exp(-2 pi i p_j k / L) in float64 (the phase
    p_j k mod L is an exact integer); e32 from the 2^20 case."""
    import torch
    from tomatis_audio_processor_amd import _lib
    p = _lib.FFT_MAX_LOG2
    L = 1 << p
    pos = np.array([0, 1, 4097, 8192 * 2048 - 1, L // 2 + 12345, L - 1, 777777, 3 * 8192 + 5],
                   np.int64)
    amp = np.array([1.0, -0.5 + 0.25j, 0.75j, 0.3 - 0.9j, -1.0, 0.6 + 0.6j, 0.2, -0.4j],
                   np.complex64)
    x = torch.zeros(L, dtype=torch.complex64, device="cuda")
    x[torch.from_numpy(pos).cuda()] = torch.from_numpy(amp).cuda()
    X = al.fft_pow2(x)
    rng = np.random.default_rng(5025)
    ks = np.unique(np.concatenate([rng.integers(0, L, 4000), [0, 1, 8191, 8192, 4095, 4096, L // 2,
                                                              L - 8192, L - 1]])).astype(np.int64)
    got = X[torch.from_numpy(ks).cuda()].cpu().numpy().astype(np.complex128)
    phase = (pos[None, :] * ks[:, None]) % L                       # exact: < 2^50
    X64 = (amp.astype(np.complex128)[None, :] * np.exp(-2j * np.pi * phase / L)).sum(axis=1)
    e = float(np.max(np.abs(got - X64)) / np.max(np.abs(X64)))
    e32 = _fft_case(20)[2]
    print(f"RATIO [fft] 2^{p} impulses: e {e:.3e} ratio {e / max(e32, cr.FLOOR):.2f}")
    assert e <= cr.bound(e32), (e, e32)


def test_fft_unsupported_lengths(al):
    import ctypes as C
    import torch
    from tomatis_audio_processor_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    for p in (3, 26, 0, -1):
        assert h.tomatis_fft_pow2_work_bytes(p) == 0
        assert h.tomatis_fft_pow2(_lib.ptr(buf), _lib.ptr(out), p, 0, _lib.ptr(buf),
                                  C.c_void_p(0)) == _lib.E_UNSUPPORTED
    for n in (8, 24, 3):
        with pytest.raises(ValueError):
            al.fft_pow2(np.zeros(n, np.complex64))


# ---------------------------------------------------------------------------
# the full correlation.  nc + nb - 1 = 16 / 17 (kMinLog: the smallest L and the
# one after it), 8192 / 8193 (kRowLog: both sides of the single-workgroup limit)
# ---------------------------------------------------------------------------
XF_CASES = [(1, 1), (5, 3), (3, 5), (9, 8), (9, 9), (5000, 3193), (5000, 3194), (3194, 5000),
            (24000, 24000), (24001, 3001)]


@pytest.mark.parametrize("nc,nb", XF_CASES)
def test_xcorr_full_against_float64(al, nc, nb):
    rng = np.random.default_rng(6000 + 31 * nc + nb)
    b = rng.standard_normal(nb).astype(np.float32)
    c = (0.5 * rng.standard_normal(nc)).astype(np.float32)
    m = min(nc, nb)
    off = (nc - m) // 3
    c[off:off + m] += b[:m]          # a coherent peak
    c64 = cr.xcorr_full(c, b, np.float64)
    c32 = fftconvolve(c, b[::-1], mode="full")
    assert c32.dtype == np.float32
    e32 = _rel(c32, c64)
    got = al.xcorr_full(c, b).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == c64.shape == (nc + nb - 1,)
    e = _rel(got, c64)
    print(f"RATIO [xcorr_full] nc {nc} nb {nb}: e {e:.3e} e32 {e32:.3e} "
          f"ratio {e / max(e32, cr.FLOOR):.2f}")
    assert e <= cr.bound(e32), (nc, nb, e, e32)
    again = al.xcorr_full(c, b).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "run-to-run"


def test_xcorr_full_over_the_cap(al):
    import ctypes as C
    import torch
    from tomatis_audio_processor_amd import _lib
    h = _lib.lib()
    cap = 1 << _lib.FFT_MAX_LOG2
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert h.tomatis_align_xcorr_full_work_bytes(cap, 2) == 0
    assert h.tomatis_align_xcorr_full_work_bytes(cap - 1, 2) > 0
    # refused before anything is read
    assert h.tomatis_align_xcorr_full(_lib.ptr(buf), cap, _lib.ptr(buf), 2, _lib.ptr(buf),
                                      _lib.ptr(buf), C.c_void_p(0)) == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        al.xcorr_full(np.zeros(0, np.float32), np.zeros(4, np.float32))


# ---------------------------------------------------------------------------
# the mean-first envelope
# ---------------------------------------------------------------------------

def _judge_mean_first(al, x, down, start, stop, name, ds_sr=None):
    import torch
    sr, ds_sr = (48000, 48000 // down) if ds_sr is None else (down * ds_sr, ds_sr)
    seg = x[start:stop]
    y64, mean64 = cr.envelope_mean_first(seg, sr, ds_sr, np.float64)
    y32, _ = cr.envelope_mean_first(seg, sr, ds_sr, np.float32)
    e32 = _rel(y32, y64)
    got, mean = al.envelope_ds(torch.from_numpy(x).cuda(), sr, ds_sr, start, stop, with_mean=True,
                               mean_first=True)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == y64.shape
    e = _rel(got, y64)
    print(f"RATIO [envelope mean-first] {name}: e {e:.3e} e32 {e32:.3e} "
          f"ratio {e / max(e32, cr.FLOOR):.2f}")
    assert e <= cr.bound(e32), (name, e, e32)
    # every float32 e[i] is within 2^-23 of its float64 value, so is their mean
    assert abs(mean - float(mean64)) <= 2.0 ** -22 * float(mean64), (name, mean, float(mean64))
    return got


@pytest.mark.parametrize("down", [24, 6])
@pytest.mark.parametrize("n", [23, 24, 25, 481, 5 * 48000 + 17])
def test_envelope_mean_first_against_resample_poly(al, n, down):
    x = white(7000 + n % 1000 + down, n, 2)
    _judge_mean_first(al, x, down, 0, n, f"len {n} down {down}")


@pytest.mark.parametrize("down", [24, 6])
def test_envelope_mean_first_subrange_of_a_resident_buffer(al, down):
    x = white(7100 + down, 9000, 2)
    got = _judge_mean_first(al, x, down, 1237, 7001, f"sub-range down {down}")
    host = al.envelope_ds(x, 48000, 48000 // down, 1237, 7001, mean_first=True).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


def test_envelope_mean_last_is_unchanged(al):
    """tomatis_align_envelope next to its new sibling: still resample_poly, then
    the mean (tests/align_ref.py), under the bound of tests/test_gpu_align.py."""
    from tests import align_ref as ar
    x = white(7200, 48000 + 17, 2)
    y64, mean64 = ar.envelope(x, 48000, 2000, np.float64)
    y32, _ = ar.envelope(x, 48000, 2000, np.float32)
    peak = float(np.max(np.abs(y64 + mean64)))
    e32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    got = al.envelope_ds(x, 48000, 2000).cpu().numpy()
    e = float(np.max(np.abs(got.astype(np.float64) - y64)) / peak)
    assert e <= ar.bound(e32), (e, e32)
    first = al.envelope_ds(x, 48000, 2000, mean_first=True).cpu().numpy()
    assert not np.array_equal(got, first)


# ---------------------------------------------------------------------------
# find_delay_full against the reference's goldens
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _inputs(pair, seed, n_base, n_target, shift):
    return make_inputs(dict(seed=seed, n_base=n_base, n_target=n_target, shift=shift))


def _case_inputs(c):
    return _inputs(c["pair"], c["seed"], c["n_base"], c["n_target"], c["shift"])


@pytest.mark.parametrize("name", [c["name"] for c in DELAY_CASES_FULL])
def test_find_delay_full_equals_reference(al, name, tmp_path):
    import torch
    from tomatis_audio_processor_amd import audio_io
    c = next(c for c in DELAY_CASES_FULL if c["name"] == name)
    fx = cr.fixture(name)
    print(f"MARGIN {name}: {float(fx['margin64']):.2e}")
    assert float(fx["margin64"]) >= MIN_MARGIN
    base, cand = _case_inputs(c)
    want = int(fx["delay"])
    assert al.find_delay_full(base, cand, sr=SR) == want
    db, dc = torch.from_numpy(np.array(base)).cuda(), torch.from_numpy(np.array(cand)).cuda()
    assert al.find_delay_full(db, dc, sr=SR) == want
    # the arg-max itself, not only the rounded delay
    b = al.envelope_ds(db, SR, 2000, mean_first=True)
    k = al.argmax_first(al.xcorr_full(al.envelope_ds(dc, SR, 2000, mean_first=True), b))
    assert (k, b.numel()) == (int(fx["k"]), int(fx["nb"]))
    pb, pc = str(tmp_path / "b.wav"), str(tmp_path / "c.wav")
    audio_io.write(pb, base, SR, "WAV", "FLOAT")
    audio_io.write(pc, cand, SR, "WAV", "FLOAT")
    assert al.find_delay_full(pb, pc, sr=SR) == want


def test_find_delay_full_host_cases(al):
    """A ratio the decimator does not take runs the reference's scipy body."""
    c = DELAY_CASES_FULL[1]
    base, cand = _case_inputs(c)
    assert not al.device_ratio(48000, 1800)
    st = cr.delay_estimate(base, cand, SR, 1800)
    assert al.find_delay_full(base, cand, sr=SR, ds_sr=1800) == st["delay"]
    assert al._find_delay_full_host(base, cand, SR, 2000) == int(cr.fixture(c["name"])["delay"])


# ---------------------------------------------------------------------------
# the residual means
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 257, 300001])
def test_residual_means(al, n):
    import torch
    from tomatis_audio_processor_amd import compare_audio as ca
    b, c = white(8000 + n % 100, n + 3, 2), white(8100 + n % 100, n + 3, 2)
    gain = np.float32(1.2345)
    db, dc = torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda()
    # rows 3.. and 1..: odd offsets into the resident buffers
    mb, mr = ca.residual_means(db[3:], dc[1:n + 1], float(gain))
    b64, c64 = b[3:].astype(np.float64), c[1:n + 1].astype(np.float64)
    pb = 0.5 * (b64 ** 2).sum(axis=1) + cr.EPS
    r = b64 - float(gain) * c64
    pr = 0.5 * (r ** 2).sum(axis=1) + cr.EPS
    # float32 elementwise, float64 sums.  power_mono(b)^2: a few roundings of 2^-24 each,
    # 2^-20 relative is 16 of them.  The residual b - gain c is off by up to 2^-23 (|b| +
    # |gain c|) per channel (two roundings), its square by twice that times |r| <= |b| +
    # |gain c|: the scale of the bound is the terms', not the difference's.
    assert abs(mb - pb.mean()) <= 2.0 ** -20 * pb.mean()
    scale = (0.5 * ((np.abs(b64) + float(gain) * np.abs(c64)) ** 2).sum(axis=1)).mean()
    assert abs(mr - pr.mean()) <= 2.0 ** -20 * scale
    assert ca.residual_means(db[3:], dc[1:n + 1], float(gain)) == (mb, mr), "run-to-run"


# ---------------------------------------------------------------------------
# compare() and main() against the reference's run
# ---------------------------------------------------------------------------
NUM = re.compile(r"-?\d+\.\d+")


@functools.lru_cache(maxsize=None)
def _main_run(name):
    """One run of main() per case: (stdout, csv header, csv columns), and of
    compare(): its return value."""
    from tomatis_audio_processor_amd import compare_audio as ca
    c = next(c for c in MAIN_CASES if c["name"] == name)
    base, cand = _case_inputs(c)
    with tempfile.TemporaryDirectory() as tmp:
        csv = os.path.join(tmp, "out.csv")
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ca.main(base, cand, n_fft=c["n_fft"], hop=c["hop"], out_csv=csv)
        with open(csv) as f:
            header = f.readline().rstrip("\n")
        cols = np.loadtxt(csv, delimiter=",", skiprows=1)
    lines = []
    ret = ca.compare(base, cand, SR, c["n_fft"], c["hop"], log=lines.append)
    return buf.getvalue(), header, cols, ret, lines


@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_main_prints_the_reference_lines(al, name):
    fx = cr.fixture(name)
    assert float(fx["margin64"]) >= MIN_MARGIN
    text, _, _, ret, lines = _main_run(name)
    want = str(fx["stdout"]).splitlines()
    got = text.splitlines()
    assert len(got) == len(want) == 8
    assert got[0] == want[0] and got[0].startswith("[ALIGN]")
    assert got[-1] == want[-1] == "[OUT] wrote diff_spectrum.csv"
    assert lines == got[:-1]                       # compare(log=...) says the same
    for g, w in zip(got[1:-1], want[1:-1]):
        assert NUM.sub("#", g) == NUM.sub("#", w)
        gv, wv = [float(v) for v in NUM.findall(g)], [float(v) for v in NUM.findall(w)]
        assert len(gv) == len(wv) >= 1
        for a, b in zip(gv, wv):
            assert abs(a - b) <= 0.01 + 1e-9, (g, w)
    assert ret[2] == int(fx["delay"])


@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_diff_spectrum_csv(al, name):
    fx = cr.fixture(name)
    c = next(c for c in MAIN_CASES if c["name"] == name)
    _, header, cols, ret, _ = _main_run(name)
    assert header == str(fx["header"]) == "freq_hz,delta_db_base_minus_cand"
    assert np.array_equal(cols[:, 0], np.fft.rfftfreq(c["n_fft"], 1 / SR))
    assert np.array_equal(cols[:, 0], fx["freqs"])
    bnd = cr.diff_db_bound(fx["b_mag"], fx["c_mag2"], MAG_RTOL)
    err = np.abs(cols[:, 1] - fx["diff_db"].astype(np.float64))
    k = int(np.argmax(err / bnd))
    print(f"RATIO [diff_db] {name}: worst error / bound {err[k] / bnd[k]:.3f} at bin {k} "
          f"({err[k]:.2e} dB of {bnd[k]:.2e} dB)")
    assert np.all(err <= bnd), (name, k, err[k], bnd[k])
    freqs, diff_db, delay, gain_db, snr_db = ret
    assert np.array_equal(diff_db.astype(np.float64), cols[:, 1]) and diff_db.dtype == np.float32
    print(f"VALUE {name}: gain_db {gain_db:.5f} (golden {float(fx['gain_db']):.5f}) "
          f"snr_db {snr_db:.5f} (golden {float(fx['snr_db']):.5f})")
    assert abs(gain_db - float(fx["gain_db"])) <= DB_ATOL
    assert abs(snr_db - float(fx["snr_db"])) <= DB_ATOL


def test_too_short_overlap_is_the_reference_error(al):
    from tomatis_audio_processor_amd import compare_audio as ca
    c = ERROR_CASES[0]
    base, cand = make_inputs(c)
    with pytest.raises(ValueError) as ei:
        ca.compare(base, cand, SR, c["n_fft"], c["hop"], log=lambda s: None)
    assert str(ei.value) == str(cr.fixture(c["name"])["error"])


def test_cli_and_step7_handoff(al, tmp_path, monkeypatch, capsys):
    """``compare_audio base cand`` writes diff_spectrum.csv into the working
    directory, and layer2b_apply_residual_eq_safe takes it."""
    from tomatis_audio_processor_amd import audio_io, compare_audio as ca
    from tomatis_audio_processor_amd import layer2b_apply_residual_eq_safe as safe
    c = MAIN_CASES[0]
    base, cand = _case_inputs(c)
    pb, pc = str(tmp_path / "base.wav"), str(tmp_path / "cand.wav")
    audio_io.write(pb, base, SR, "WAV", "FLOAT")
    audio_io.write(pc, cand, SR, "WAV", "FLOAT")
    monkeypatch.chdir(tmp_path)
    ca._cli([pb, pc])
    out = capsys.readouterr().out
    assert out.splitlines()[0] == str(cr.fixture(c["name"])["stdout"]).splitlines()[0]
    csv = tmp_path / "diff_spectrum.csv"
    assert csv.exists()
    short = str(tmp_path / "in.wav")
    audio_io.write(short, cand[:SR], SR, "WAV", "PCM_24")
    safe.main(["--in_audio", short, "--out_audio", str(tmp_path / "out.flac"),
               "--diff_csv", str(csv)])
    assert "[DONE]" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        ca.main(pb, pc, sr=44100, out_csv=str(tmp_path / "x.csv"))
