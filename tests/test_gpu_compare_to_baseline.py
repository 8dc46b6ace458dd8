"""GPU: compare_to_baseline on the device: the fused mean
log-power spectrum (tm_analysis.hip), the time-domain sums (tm_align.hip) and
``compare_to_baseline``'s functions, ``compare_many`` and ``main`` against the
reference's goldens (tools/make_baseline_goldens.py).

The spectrum is judged by the rule of tests/compare_ref.bound moved to dB: with
the float64 numpy statement S64 of avg_spectrum_db and the reference's own
float32 result S32 of it (tests/baseline_ref.py),

    max |S - S64|  <=  8 * max(e32, spacing(float32(max |S64|))),  e32 = max |S32 - S64|.

The sums are judged like tomatis_compare_residual (2^-20 relative), delays as
integers after the stored float64 margin of the correlation's top is shown to be
>= 1e-3 (the single-lag pair: inf).

Largest measured max |S - S64| / max(e32, spacing) on the MI355X (the float64
output of the kernel; the bound is 8): 4.06 (3000 / 750, F = 18), 3.28 (256 / 64,
F = 33), 0.99 to 2.72 on the other shapes.  CSV columns of the fixtures: at most
0.45 of their bound (``delta_raw`` of the 12 s pair), 0.29 on the 40 s pairs; the
three sums at most 0.08 of theirs.  Before the two real bins (0 and n / 2) were
summed in float64, bin n / 2 alone missed: 9.79 at 256 / 64, F = 7, and 1.04 of
the column bound on the first 40 s pair.
"""
import contextlib
import functools
import io
import os
import re
import tempfile

import numpy as np
import pytest

from tests import baseline_ref as br
from tests.golden.baseline_cases import (BASELINE_FILE, ERROR_CASES, MAIN_CASES, MIN_MARGIN, OUTDIR,
                                         SR, make_inputs)
from tests.stft_ref import white

pytestmark = pytest.mark.gpu

DB_ATOL = 2e-3    # tests/test_gpu_compare.py: dB
SLAB = 16         # frames per slab: 2 * kSlabPairs of tm_analysis.hip
BAND_KEYS = [k for k, _, _ in br.BANDS]


@pytest.fixture(scope="module")
def cb():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, compare_to_baseline
    _lib.lib()
    return compare_to_baseline


# ---------------------------------------------------------------------------
# the fused spectrum against the float64 statement
# ---------------------------------------------------------------------------
# (n_fft, hop, F, mode, scale): one frame; an odd count inside one slab; two
# slabs and one unpaired frame in a third; the smallest and the largest
# transform; Bluestein lengths (one with more than a slab, an even count); a
# scale; raw mono; the reference's default transform with more than two slabs
SPEC_CASES = [
    (256, 64, 1, "pm", 1.0),
    (256, 64, 7, "pm", 1.0),
    (256, 64, 2 * SLAB + 1, "pm", 1.0),
    (16, 4, 3, "pm", 1.0),
    (16384, 4096, 3, "pm", 1.0),
    (1000, 250, 5, "pm", 1.0),
    (3000, 750, SLAB + 2, "pm", 1.0),
    (256, 64, SLAB + 4, "pm", 0.37),
    (512, 128, 9, "raw", 1.0),
    (4096, 2048, 2 * SLAB + 3, "pm", 1.0),
]


def _signal(seed, n, ch):
    """Seeded noise with a tone, a few samples more than the frames need."""
    t = np.arange(n, dtype=np.float64)
    tone = 0.3 * np.sin(2 * np.pi * 997.0 / SR * t)
    x = white(seed, n, ch, amp=0.1).astype(np.float64) + tone[:, None] * np.array([1.0, 0.7])[:ch]
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _spec_case(n_fft, hop, F, mode, scale):
    """-> (x, S64, e32, bound)."""
    n = n_fft + (F - 1) * hop + min(hop - 1, 3)
    x = _signal(5100 + n_fft + F, n, 2 if mode == "pm" else 1)
    s32 = np.float32(scale)
    if mode == "pm":
        m32 = br.power_mono(x * s32)
        m64 = br.power_mono(x.astype(np.float64) * float(s32), np.float64)
    else:
        m32 = x[:, 0] * s32
        m64 = x[:, 0].astype(np.float64) * float(s32)
    S64 = br.avg_spectrum_db(m64, n_fft, hop, np.float64)
    S32 = br.avg_spectrum_db(m32, n_fft, hop, np.float32).astype(np.float32)
    e32 = float(np.max(np.abs(S32.astype(np.float64) - S64)))
    return x, S64, e32, br.db_bound(e32, np.max(np.abs(S64)))


@pytest.mark.parametrize("n_fft,hop,F,mode,scale", SPEC_CASES)
def test_spectrum_mean_against_float64(cb, n_fft, hop, F, mode, scale):
    import torch
    from tomatis_audio_processor_amd import analysis
    x, S64, e32, bnd = _spec_case(n_fft, hop, F, mode, scale)
    assert analysis._n_frames(len(x), n_fft, hop) == F
    if mode == "pm":
        xd, sig, ch = torch.from_numpy(x).cuda(), analysis.AN_SIG_POWER_MONO, 2
    else:
        xd, sig, ch = torch.from_numpy(x[:, 0].copy()).cuda(), analysis.AN_SIG_RAW, 1
    got = cb.spectrum_mean(xd, n_fft, hop, sig, ch, scale).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == S64.shape == (n_fft // 2 + 1,)
    err = np.abs(got - S64)
    k = int(np.argmax(err))
    print(f"RATIO [spectrum_mean] {n_fft}/{hop} F {F} {mode} scale {scale}: worst error / "
          f"max(e32, spacing) {err[k] / (bnd / br.FACTOR):.2f} at bin {k} ({err[k]:.2e} dB, e32 "
          f"{e32:.2e} dB, bound {bnd:.2e} dB)")
    assert err[k] <= bnd, (n_fft, hop, F, k, err[k], bnd)
    again = cb.spectrum_mean(xd, n_fft, hop, sig, ch, scale).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "run-to-run"
    if scale == 1.0:  # the public function: the float32 cast of the same numbers
        freqs, S = cb.avg_spectrum_db(x if mode == "pm" else x[:, 0], SR, n_fft, hop)
        assert freqs.dtype == S.dtype == np.float32
        assert np.array_equal(freqs, np.fft.rfftfreq(n_fft, 1.0 / SR).astype(np.float32))
        assert np.array_equal(S, got.astype(np.float32))
        assert np.max(np.abs(S.astype(np.float64) - S64)) <= bnd


def test_spectrum_mean_does_not_depend_on_what_follows_the_last_frame(cb):
    """An odd count's missing partner adds nothing: the samples after the last
    frame (fewer than a hop) do not move a bit."""
    import torch
    from tomatis_audio_processor_amd import analysis
    x, _, _, _ = _spec_case(256, 64, 2 * SLAB + 1, "pm", 1.0)
    n = 256 + 2 * SLAB * 64
    a = cb.spectrum_mean(torch.from_numpy(x[:n].copy()).cuda(), 256, 64,
                         analysis.AN_SIG_POWER_MONO, 2).cpu().numpy()
    y = x.copy()
    y[n:] = 0.9
    b = cb.spectrum_mean(torch.from_numpy(y).cuda(), 256, 64, analysis.AN_SIG_POWER_MONO,
                         2).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_spectrum_mean_refusals(cb):
    import ctypes as C
    import torch
    from tomatis_audio_processor_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    dbl = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p, q, st = _lib.ptr(buf), _lib.ptr(dbl), C.c_void_p(0)
    one = C.c_float(1.0)
    # before anything is read: a length the LDS does not hold, channels against the mode
    assert h.tomatis_an_spectrum_mean(p, 2048, 2, 8, 4, 1, one, p, q, q, st) == _lib.E_UNSUPPORTED
    assert h.tomatis_an_spectrum_mean(p, 2048, 2, 9000, 4, 1, one, p, q, q, st) == \
        _lib.E_UNSUPPORTED
    assert h.tomatis_an_spectrum_mean(p, 2048, 1, 256, 64, 1, one, p, q, q, st) == _lib.E_ARG
    assert h.tomatis_an_spectrum_mean(p, 2048, 2, 256, 64, 0, one, p, q, q, st) == _lib.E_ARG
    assert h.tomatis_an_spectrum_mean(p, 2048, 2, 256, 0, 1, one, p, q, q, st) == _lib.E_ARG
    with pytest.raises(ValueError, match="segment too short"):
        cb.avg_spectrum_db(np.zeros((255, 2), np.float32), SR, 256, 64)
    with pytest.raises(ValueError):
        cb.avg_spectrum_db(np.zeros((64, 2), np.float32), SR, 8, 4)


# ---------------------------------------------------------------------------
# the time-domain sums
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pair12():
    return make_inputs(MAIN_CASES[2])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 12 * SR])
def test_mono_sums(cb, n):
    import torch
    if n == 12 * SR:
        base, (cand,) = _pair12()
        b, c = np.concatenate([base[:3], base]), np.concatenate([cand[:1], cand])
    else:
        b, c = white(8200 + n % 100, n + 3, 2), white(8300 + n % 100, n + 3, 2)
    gain = np.float32(1.2345)
    db, dc = torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda()
    # rows 3.. and 1..: odd offsets into the resident buffers
    got = cb.mono_sums(db[3:], dc[1:n + 1], float(gain))
    want = br.mono_sums(b[3:], c[1:n + 1], float(gain), np.float64)
    mb, mc = br.power_mono(b[3:], np.float64), br.power_mono(c[1:n + 1], np.float64)
    # float32 elementwise, float64 sums.  mb^2, mc^2: a few roundings of 2^-24 each, 2^-20
    # relative is 16 of them.  The difference mb - g mc is off by up to 2^-23 (mb + g mc) (the
    # monos', the product's and its own rounding), its square by twice that times |r| <= mb +
    # g mc: the scale of the third bound is the terms', not the difference's.
    scale = (float(np.sum(mb * mb)), float(np.sum(mc * mc)),
             float(np.sum((mb + float(gain) * mc) ** 2)))
    for name, g, w, s in zip(("sum mb^2", "sum mc^2", "sum resid^2"), got, want, scale):
        print(f"RATIO [mono_sums] n {n} {name}: {abs(g - float(w)) / (2.0 ** -20 * s):.3f}")
        assert abs(g - float(w)) <= 2.0 ** -20 * s, (n, name, g, float(w))
    assert cb.mono_sums(db[3:], dc[1:n + 1], float(gain)) == got, "run-to-run"
    # the first call of compute_metrics: no gain, the third sum is sum mb^2's twin
    g0 = cb.mono_sums(db[3:], dc[1:n + 1])
    assert g0[:2] == got[:2] and g0[2] == g0[0]


# ---------------------------------------------------------------------------
# compare_many / main against the reference's run
# ---------------------------------------------------------------------------
NUM = re.compile(r"[-+]?\d+\.\d+")


@contextlib.contextmanager
def _files(c):
    """The case's files in a temporary working directory, named as in the golden run."""
    from tomatis_audio_processor_amd import audio_io
    base, cands = make_inputs(c)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            audio_io.write(BASELINE_FILE, base, SR, "WAV", "FLOAT")
            for k, x in zip(c["cands"], cands):
                audio_io.write(k["file"], x, k.get("sr", SR), "WAV", "FLOAT")
            yield tmp
        finally:
            os.chdir(cwd)


def _argv(c):
    return ["--baseline", BASELINE_FILE, "--candidates", *[k["file"] for k in c["cands"]],
            "--outdir", OUTDIR, "--n_fft", str(c["n_fft"]), "--hop", str(c["hop"]),
            "--max_minutes", str(c["max_minutes"])]


@functools.lru_cache(maxsize=None)
def _main_run(name):
    """One run of main() per case -> (stdout, summary.txt, [(header, columns)],
    sizes of the files in the output directory, compare_many's results)."""
    from tomatis_audio_processor_amd import compare_to_baseline as cb
    c = next(c for c in MAIN_CASES if c["name"] == name)
    with _files(c):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            cb.main(_argv(c))
        with open(os.path.join(OUTDIR, "summary.txt"), encoding="utf-8") as f:
            summary = f.read()
        csvs = []
        for k in c["cands"]:
            p = os.path.join(OUTDIR, "diff_" + os.path.splitext(k["file"])[0] + ".csv")
            with open(p) as f:
                header = f.readline().rstrip("\n")
            csvs.append((header, np.loadtxt(p, delimiter=",", skiprows=1)))
        sizes = {p: os.path.getsize(os.path.join(OUTDIR, p)) for p in os.listdir(OUTDIR)}
        with contextlib.redirect_stdout(io.StringIO()):
            results = cb.compare_many(BASELINE_FILE, [k["file"] for k in c["cands"]], OUTDIR, SR,
                                      c["n_fft"], c["hop"], c["max_minutes"])
    for r in results:  # the resident segments are not needed any more
        r.pop("xb_seg"), r.pop("xc_seg")
    return buf.getvalue(), summary, csvs, sizes, results


def _same_text(got, want):
    """Line for line with the numbers masked; every number within 0.01."""
    got, want = got.splitlines(), want.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert NUM.sub("#", g) == NUM.sub("#", w), (g, w)
        gv, wv = [float(v) for v in NUM.findall(g)], [float(v) for v in NUM.findall(w)]
        assert len(gv) == len(wv)
        for a, b in zip(gv, wv):
            assert abs(a - b) <= 0.01 + 1e-9, (g, w)


@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_main_writes_the_reference_texts(cb, name):
    c = next(c for c in MAIN_CASES if c["name"] == name)
    fx = br.fixture(name)
    text, summary, csvs, sizes, results = _main_run(name)
    _same_text(summary, str(fx["summary"]))
    _same_text(text, str(fx["stdout"]))
    # the lines without a number in them are the golden's own
    assert summary.splitlines()[:3] == str(fx["summary"]).splitlines()[:3]
    assert text == str(fx["stdout"])
    stems = [os.path.splitext(k["file"])[0] for k in c["cands"]]
    assert set(sizes) == {"summary.txt", "delta_overlay.png", "env_rms_dbfs.png",
                          *[f"diff_{s}.csv" for s in stems]}
    assert [r["name"] for r in results] == stems
    assert [r["path"] for r in results] == [k["file"] for k in c["cands"]]
    pytest.importorskip("matplotlib")
    assert sizes["delta_overlay.png"] > 0 and sizes["env_rms_dbfs.png"] > 0


@pytest.mark.parametrize("name", [c["name"] for c in MAIN_CASES])
def test_delays_columns_and_metrics(cb, name):
    c = next(c for c in MAIN_CASES if c["name"] == name)
    fx = br.fixture(name)
    _, _, csvs, _, results = _main_run(name)
    assert len(results) == int(fx["n_cands"])
    for i, (r, (header, cols)) in enumerate(zip(results, csvs)):
        print(f"MARGIN {name}[{i}]: {float(fx[f'margin64_{i}']):.2e}")
        assert float(fx[f"margin64_{i}"]) >= MIN_MARGIN
        assert r["delay"] == int(fx[f"delay_{i}"])
        assert header == str(fx["header"]) == br.CSV_HEADER
        want = fx[f"cols_{i}"]
        assert np.array_equal(cols[:, 0], want[:, 0].astype(np.float64))
        assert np.array_equal(cols[:, 0],
                              np.fft.rfftfreq(c["n_fft"], 1.0 / SR).astype(np.float32))
        # a column is the difference of two spectra (or a mean of such differences): the two
        # spectra's bounds added, i.e. twice the spectrum bound
        bnd = sum(br.db_bound(e, s) for e, s in zip(fx[f"e32_{i}"], fx[f"smax_{i}"]))
        for j, col in ((1, "delta_raw"), (2, "delta_anch"), (3, "delta_smooth")):
            err = np.abs(cols[:, j] - want[:, j].astype(np.float64))
            k = int(np.argmax(err))
            print(f"RATIO [{col}] {name}[{i}]: worst error / bound {err[k] / bnd:.3f} at bin {k} "
                  f"({err[k]:.2e} dB of {bnd:.2e} dB)")
            assert err[k] <= bnd, (name, i, col, k, err[k], bnd)
            assert np.array_equal(cols[:, j], r[col].astype(np.float64))
            assert r[col].dtype == np.float32
        vals = dict(gain_db=r["gain_db"], anchor=r["anchor_db"], snr=r["snr"],
                    music_err=r["music_err"], noise_delta=r["noise_delta"])
        for key, v in vals.items():
            print(f"VALUE {name}[{i}] {key}: {v:.5f} (golden {float(fx[f'{key}_{i}']):.5f})")
            assert abs(v - float(fx[f"{key}_{i}"])) <= DB_ATOL, (name, i, key)
        for key, w in zip(BAND_KEYS, fx[f"stats_{i}"]):
            assert abs(r["stats"][key] - float(w)) <= DB_ATOL, (name, i, key)


def test_functions_on_arrays_tensors_and_paths(cb):
    """find_delay_by_corr, get_aligned_overlap and compute_metrics on their own,
    on every kind of input, equal what compare_many made of the files."""
    import torch
    name = "baseline_m3210_1024"
    c = next(c for c in MAIN_CASES if c["name"] == name)
    want = _main_run(name)[4][0]
    base, (cand,) = make_inputs(c)
    db, dc = torch.from_numpy(base).cuda(), torch.from_numpy(cand).cuda()
    assert cb.find_delay_by_corr(cand, base, SR) == want["delay"]
    assert cb.find_delay_by_corr(dc, db) == want["delay"]
    b, x, delay = cb.get_aligned_overlap(db, dc, SR, c["max_minutes"])
    assert delay == want["delay"] == -3216
    n = int(c["max_minutes"] * 60 * SR)
    assert b.shape == x.shape == (n, 2)
    assert b.data_ptr() == db[3216:].data_ptr() and x.data_ptr() == dc.data_ptr()   # no copy
    uncapped = cb.get_aligned_overlap(base, cand, SR)[0]
    assert uncapped.shape[0] == min(len(base) - 3216, len(cand))
    m = cb.compute_metrics(b, x, SR, c["n_fft"], c["hop"])
    assert len(m) == 10
    for got, key in zip(m[:4], ("freqs", "delta_raw", "delta_anch", "delta_smooth")):
        assert np.array_equal(got, want[key])
    assert m[4:6] == (want["gain_db"], want["anchor_db"]) and m[6] == want["stats"]
    assert (m[7], m[8], m[9]) == (want["music_err"], want["noise_delta"], want["snr"])
    with _files(c):
        assert cb.find_delay_by_corr(c["cands"][0]["file"], BASELINE_FILE) == want["delay"]


@pytest.mark.parametrize("name", [c["name"] for c in ERROR_CASES])
def test_error_cases_raise_the_reference_message(cb, name):
    c = next(c for c in ERROR_CASES if c["name"] == name)
    with _files(c):
        with pytest.raises(ValueError) as ei:
            cb.main(_argv(c))
        assert not os.path.exists(os.path.join(OUTDIR, "summary.txt"))
    assert str(ei.value) == str(br.fixture(name)["error"])


# ---------------------------------------------------------------------------
# the envelope
# ---------------------------------------------------------------------------

def test_frame_rms_dbfs(cb):
    import torch
    base, _ = _pair12()
    x = base[SR:2 * SR]
    mono = br.power_mono(x)
    win, hop = 2400, 1200          # 50 ms / 25 ms at 48 kHz
    F = 1 + (len(x) - win) // hop
    r = np.array([np.sqrt(np.mean(mono[i * hop:i * hop + win] ** 2) + br.EPS) for i in range(F)],
                 np.float32)
    got = cb.frame_r(torch.from_numpy(x.copy()).cuda(), win, hop)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), r.view(np.uint32))
    t, y = cb.frame_rms_dbfs(torch.from_numpy(x.copy()).cuda(), SR)
    assert t.dtype == y.dtype == np.float32 and t.shape == y.shape == (F,)
    assert np.array_equal(t, ((np.arange(F) * hop) / SR).astype(np.float32))
    want = np.array([cb.rms_dbfs_from_mono(mono[i * hop:i * hop + win]) for i in range(F)],
                    np.float32)
    # log10 of the same float32 r, as an array here and a scalar there: an ulp of dB
    assert np.max(np.abs(y - want)) <= 2 * np.spacing(np.float32(np.max(np.abs(want))))
    # shorter than one window: the reference's one-point answer
    t, y = cb.frame_rms_dbfs(torch.from_numpy(x[:win - 1].copy()).cuda(), SR)
    assert np.array_equal(t, np.array([0.0])) and y.shape == (1,)
    assert y[0] == cb.rms_dbfs_from_mono(mono[:win - 1])
    assert cb.frame_rms_dbfs(x[:100], SR, 1, 1)[1][0] == cb.rms_dbfs_from_mono(mono[:100])
