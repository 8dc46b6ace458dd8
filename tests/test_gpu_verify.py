"""GPU: the acceptance validators on the device.

* the new kernels against tests/verify_ref.py in float64 under the project's
  rule ``err <= 8 * max(e32, 2^-23)``, ``e32`` being the float32 numpy
  statement's own error on the same input;
* the float64 sum against ``math.fsum``;
* every exact quantity (levels, thresholds, states, counts, peak) and every
  toleranced one (spectra, DC, tilt index, printed text) on every fixture
  recorded from the reference's own runs;
* the package's own CLIs end to end.
"""
import contextlib
import io
import math
import os
import re

import numpy as np
import pytest

from tests import verify_ref as vr
from tests.golden import verify_cases as vc
from tests.golden_util import load_fixture, sha

pytestmark = pytest.mark.gpu
DB_ATOL = 2e-3       # dB, conditional spectra (tests/test_gpu_analysis.py)
TI_ATOL = 1e-3       # dB, tilt-index means and standard deviations
SR = 48000


def _mods():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import analysis, validate_layer1, verify_tomatis_15db_v2
    return torch, analysis, verify_tomatis_15db_v2, validate_layer1


# ---------------------------------------------------------------------------
# kernels against the float64 statement
# ---------------------------------------------------------------------------

def _signal(seed, n, ch):
    """x: enveloped noise; y: x through a first difference (a tilt), so that the
    ratio rows are far from flat."""
    x = vc.make_x(dict(x="env", seed=seed, ch=ch))[:n]
    y = x.copy()
    y[1:] -= np.float32(0.9) * x[:-1]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


# name -> (n_fft, hop, ch, n): n is chosen so that the frame counts cover 1, odd and even
SHAPES = {
    "4096_2048_st": (4096, 2048, 2, SR * 4 + 11),        # 17 anchor bins
    "256_64_st": (256, 64, 2, 256 + 64 * 40 + 5),        # one anchor bin, 4 and 32 band bins
    "3000_750_mono": (3000, 750, 1, SR * 4 + 7),         # Bluestein, 12 anchor bins
    "64_16_st": (64, 16, 2, 64 + 16 * 36 + 3),           # no anchor bin, one-bin low band
    "16384_4096_mono": (16384, 4096, 1, SR * 4),         # the LDS ceiling
    "16384_4096_st": (16384, 4096, 2, 16384 + 4096 * 3 + 5),   # and its largest register budget
    "one_frame": (4096, 2048, 2, 4096 + 100),            # F = 1
}
ANCHOR_BINS = {"4096_2048_st": 17, "256_64_st": 1, "3000_750_mono": 12, "64_16_st": 0,
               "16384_4096_mono": 68, "16384_4096_st": 68, "one_frame": 17}


def _bins(n_fft):
    freqs = np.fft.rfftfreq(n_fft, 1 / SR)
    return (vr.band_bins(freqs, 900, 1100), vr.band_bins(freqs, 200, 1000),
            vr.band_bins(freqs, 2000, 8000))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_and_bands_against_float64(shape):
    torch, A, _, _ = _mods()
    n_fft, hop, ch, n = SHAPES[shape]
    x, y = _signal(311, n, ch)
    anchor, lo, hi = _bins(n_fft)
    assert anchor[1] - anchor[0] == ANCHOR_BINS[shape]
    if shape == "256_64_st":
        assert (lo[1] - lo[0], hi[1] - hi[0]) == (4, 32)
    if shape == "64_16_st":
        assert lo[1] - lo[0] == 1
    xd, yd = A.pair_on_device(x, y, 0)
    rows, be = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(*lo, *hi), fused=True)
    rows2, be2 = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(*lo, *hi), fused=True)
    rows_u, be_u = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(*lo, *hi),
                                    fused=False)
    torch.cuda.synchronize()
    F = vr.n_inside(n, n_fft, hop)
    assert rows.shape == (F, n_fft // 2 + 1) and be.shape == (F, 4)
    if shape == "one_frame":
        assert F == 1
    # two calls, and the fused and the unfused form, agree bit for bit
    assert torch.equal(rows, rows2) and torch.equal(be, be2)
    assert torch.equal(rows, rows_u) and torch.equal(be, be_u)
    rows, be = rows.cpu().numpy().astype(np.float64), be.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(be))

    r64, X64, Y64 = vr.ratio_rows(x, y, n_fft, hop, *anchor, dtype=np.float64)
    r32, _, _ = vr.ratio_rows(x, y, n_fft, hop, *anchor, dtype=np.float32)
    ok = (X64 >= 1e-3 * X64.max(axis=1, keepdims=True)) & \
         (Y64 >= 1e-3 * Y64.max(axis=1, keepdims=True))
    assert np.count_nonzero(~ok) <= 1e-3 * ok.size, np.count_nonzero(~ok)
    e32 = float(np.max(np.abs(r32.astype(np.float64) - r64)[ok] / r64[ok]))
    err = float(np.max(np.abs(rows - r64)[ok] / r64[ok]))
    print(f"{shape}: rows err {err:.2e} e32 {e32:.2e} left out {np.count_nonzero(~ok)}/{ok.size}")
    assert err <= vr.rule_bound(e32), (err, e32)

    b64 = vr.band_energies(x, y, n_fft, hop, *lo, *hi, dtype=np.float64)
    b32 = vr.band_energies(x, y, n_fft, hop, *lo, *hi, dtype=np.float32).astype(np.float64)
    scale = np.repeat(np.stack([b64[:, :2].max(axis=1), b64[:, 2:].max(axis=1)], axis=1), 2, axis=1)
    e32b = float(np.max(np.abs(b32 - b64) / scale))
    errb = float(np.max(np.abs(be - b64) / scale))
    print(f"{shape}: bands err {errb:.2e} e32 {e32b:.2e}")
    assert errb <= vr.rule_bound(e32b), (errb, e32b)

    if anchor[0] == anchor[1]:
        # no anchor bin: the rows are TOMATIS_AN_RATIO's, bit for bit
        plain = A._spectra(xd, yd, n, ch, n_fft, hop, A.AN_RATIO, A.AN_SIG_RAW)
        assert torch.equal(plain, rows_u)


def test_odd_frame_count_and_single_calls():
    torch, A, _, _ = _mods()
    n_fft, hop, ch = 256, 64, 2
    n = n_fft + hop * 6 + 9                      # F = 7
    x, y = _signal(312, n, ch)
    anchor, lo, hi = _bins(n_fft)
    xd, yd = A.pair_on_device(x, y, 0)
    rows, be = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(*lo, *hi))
    only_rows, none = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor)
    none2, only_be = A.verify_spectra(xd, yd, n_fft, hop, bands=(*lo, *hi))
    assert rows.shape[0] == 7 and none is None and none2 is None
    assert torch.equal(rows, only_rows) and torch.equal(be, only_be)


def test_zero_anchor_leaves_the_row_unscaled_and_empty_bands_sum_to_zero():
    torch, A, _, _ = _mods()
    n_fft = hop = 256                             # frames do not overlap
    n = n_fft * 6
    x, y = _signal(313, n, 2)
    y[3 * n_fft:4 * n_fft] = 0                    # frame 3: Y = 0 in the anchor band (everywhere)
    anchor, lo, hi = _bins(n_fft)
    xd, yd = A.pair_on_device(x, y, 0)
    rows, be = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(lo[0], lo[0], 7, 7))
    plain = A._spectra(xd, yd, n, 2, n_fft, hop, A.AN_RATIO, A.AN_SIG_RAW)
    torch.cuda.synchronize()
    assert torch.equal(rows[3], plain[3]) and float(rows[3].abs().max()) == 0.0   # g = 0
    assert not torch.equal(rows[2], plain[2])                                      # g > 0: scaled
    a = rows[2, anchor[0]:anchor[1]].cpu().numpy()
    assert abs(float(a.mean()) - 1.0) < 1e-6      # the anchor band's mean gain is 1
    assert float(be.abs().max()) == 0.0           # both ranges empty
    # a range the binding refuses: no launch
    with pytest.raises(RuntimeError):
        A.verify_spectra(xd, yd, n_fft, hop, anchor=(5, n_fft))


@pytest.mark.parametrize("n,ch", [(1, 1), (255, 1), (256 * 1024 + 3, 1), (50001, 2)])
def test_float64_sum(n, ch):
    torch, A, _, _ = _mods()
    rng = np.random.default_rng(n)
    v = (rng.standard_normal((n, ch)) * 0.1 + 0.002).astype(np.float32)
    t = torch.from_numpy(v).cuda()
    s1, s2 = A.sum_f64(t), A.sum_f64(t)
    want = math.fsum(v.reshape(-1).astype(np.float64).tolist())
    assert s1 == s2                                # the same bits in every run
    assert abs(s1 - want) <= 1e-12 * abs(want), (s1, want)
    assert A.absmax(t) == np.max(np.abs(v))


# ---------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------

_NUM = re.compile(r"(-?\d+(?:\.\d+)?)")
# The printed lines that carry a toleranced quantity, and its tolerance; every
# other line (T, shares, levels, level differences, peak, counts, words) is
# derived from exact quantities and is compared as text.
_TOLERANCED = [
    (re.compile(r"DC偏移"), 2.0 ** -20 * 1e-2),                       # 2^-20 relative, |dc| < 0.01
    (re.compile(r"RMSE=|^    C1: .* dB, C2: .* dB$|^    (low|mid|high) \("), DB_ATOL),
    (re.compile(r" TI \(n=|C[12] TI:"), TI_ATOL),
    (re.compile(r"分离度"), 2 * TI_ATOL),                             # a difference of two means
]


def _same_text(got, want):
    """Line for line.  A line of _TOLERANCED: words and integers exactly, each
    decimal within the line's tolerance plus one unit of its last printed digit
    (two values that close may round to neighbouring digits).  Any other line:
    the same text."""
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (len(g), len(w))
    for a, b in zip(g, w):
        tol = next((t for rx, t in _TOLERANCED if rx.search(b)), None)
        if tol is None:
            assert a == b, (a, b)
            continue
        pa, pb = _NUM.split(a), _NUM.split(b)
        assert pa[0::2] == pb[0::2], (a, b)
        for u, v in zip(pa[1::2], pb[1::2]):
            if "." in v:
                k = len(v.split(".")[1])
                assert "." in u and abs(float(u) - float(v)) <= tol + 10.0 ** -k + 1e-12, (a, b)
            else:
                assert u == v, (a, b)


def _typed(parser, a, extra=()):
    """The argument dict as the CLI's argparse types it (``--fc 1000`` is 1000.0):
    the fixtures' runs passed every flag on the command line."""
    argv = ["-i", "x", "-o", "y", *extra]
    for k, v in a.items():
        argv += ["--" + k, str(v)]
    ns = vars(parser.parse_args(argv))
    return {k: ns[k] for k in a}


def _run(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


@pytest.mark.parametrize("name", [c["name"] for c in vc.V2_CASES])
def test_v2_fixture(name, tmp_path, monkeypatch):
    torch, A, v2, _ = _mods()
    c, fx = vc.BY_NAME[name], load_fixture(name)
    x, y, _ = vc.make_pair(c)
    assert sha(x) == str(fx["x_sha"])
    a = _typed(v2.build_parser(), vc.v2_args(c))
    monkeypatch.chdir(tmp_path)
    R, text = _run(v2.verify, x, y, SR, **a)

    # exact: levels, threshold, share, states, counts, peak, exit code
    assert sha(np.ascontiguousarray(R["levels"], np.float64)) == str(fx["levels_sha"])
    assert float(R["optimal_T"]) == float(fx["T"]) and R["achieved_c2"] == float(fx["ratio"])
    assert vr.state_sha(R["codes"]) == str(fx["state_sha"])
    assert R["stats"]["switch_count"] == int(fx["switch_count"])
    cls = A.stable_classes(R["codes"])
    assert [int(np.count_nonzero(cls == 1)), int(np.count_nonzero(cls == 2))] == \
        fx["stable"].tolist()
    assert [R["c1_n"], R["c2_n"]] == fx["used"].tolist()
    keys = ("input", "output", "c1", "c2")
    assert [len(R["ti_data"][k]) for k in keys] == fx["ti_n"].tolist()
    assert np.float32(R["eng"]["peak"]).view(np.uint32) == fx["peak_bits"]
    assert R["exit_code"] == int(fx["exit_code"])

    # toleranced: spectra, DC, tilt index
    cols = np.stack([R["c1_db"], R["c1_theory"], R["c2_db"], R["c2_theory"]], axis=1)
    err = float(np.max(np.abs(cols - fx["cols"].astype(np.float64))))
    print(f"{name}: spectra err {err:.2e} dB")
    assert err <= DB_ATOL, err
    dc = float(fx["dc"])
    assert abs(R["eng"]["dc_mean"] - dc) <= 2.0 ** -20 * abs(dc)
    for i, k in enumerate(keys):
        if fx["ti_n"][i]:
            assert abs(float(R["ti"][k + "_mean"]) - fx["ti_mean"][i]) <= TI_ATOL, k
            assert abs(float(R["ti"][k + "_std"]) - fx["ti_std"][i]) <= TI_ATOL, k

    # the printed text, the report and the files
    _same_text(text, str(fx["stdout"]))
    _same_text(R["report"], str(fx["report"]))
    for suffix in ("_spectrum.csv", "_spectrum.png", "_tilt_index.png", "_report.txt"):
        assert os.path.getsize(a["out_prefix"] + suffix) > 0
    assert open(a["out_prefix"] + "_report.txt", encoding="utf-8").read() == R["report"]
    got = np.loadtxt(a["out_prefix"] + "_spectrum.csv", delimiter=",", skiprows=1)
    assert np.array_equal(got[:, 0], fx["freq_col"])
    assert float(np.max(np.abs(got[:, 1:] - fx["cols"]))) <= DB_ATOL


@pytest.mark.parametrize("name", [c["name"] for c in vc.V2_CASES])
def test_v2_gate_functions(name):
    """compute_frame_levels, find_optimal_threshold and
    simulate_gate_with_threshold on their own, up-delay 0 and 100 ms."""
    torch, A, v2, _ = _mods()
    c = vc.BY_NAME[name]
    x, _, _ = vc.make_pair(c)
    want, _ = vr.frame_levels(x, c["n_fft"], c["hop"])
    levels = v2.compute_frame_levels(x, SR, c["n_fft"], c["hop"])
    assert levels.dtype == np.float64 and np.array_equal(levels, want)   # bit-identical
    for ms, hyst in ((0, 1.0), (100.0, 3.0)):
        udf = int(ms * SR / 1000 / c["hop"])
        T, ratio = v2.find_optimal_threshold(levels, hyst, 0.5, udf)
        assert (T, ratio) == vr.find_optimal_threshold(want, hyst, 0.5, udf)
        states = v2.simulate_gate_with_threshold(levels, T, hyst, udf)
        assert states == A.state_names(vr.gate_frames(want, T, hyst, udf))


@pytest.mark.parametrize("name", [c["name"] for c in vc.L1_CASES])
def test_l1_fixture(name, tmp_path, monkeypatch):
    torch, A, _, l1 = _mods()
    c, fx = vc.BY_NAME[name], load_fixture(name)
    x, y, rows = vc.make_pair(c)
    assert sha(x) == str(fx["x_sha"])
    a = _typed(l1.build_parser(), vc.l1_args(c), ("--state_csv", "s"))
    monkeypatch.chdir(tmp_path)
    R, text = _run(l1.validate, x, y, SR, vc.csv_frames(rows), **a)
    assert sha(np.ascontiguousarray(R["sim_levels"], np.float64)) == str(fx["levels_sha"])
    assert vr.state_sha(R["sim_codes"]) == str(fx["state_sha"])
    cmp = R["cmp"]
    assert (cmp["mismatch_count"], cmp["total_frames"], cmp["csv_switches"],
            cmp["sim_switches"]) == (int(fx["mismatch"]), int(fx["total"]),
                                     int(fx["csv_switches"]), int(fx["sim_switches"]))
    assert cmp["level_max_diff"] == float(fx["level_max_diff"])
    assert [R["c1_n"], R["c2_n"]] == fx["used"].tolist()
    assert np.float32(R["eng"]["peak"]).view(np.uint32) == fx["peak_bits"]
    assert R["exit_code"] == int(fx["exit_code"])
    cols = np.stack([R["c1_db"], R["c1_theory"], R["c2_db"], R["c2_theory"]], axis=1)
    err = float(np.max(np.abs(cols - fx["cols"].astype(np.float64))))
    print(f"{name}: spectra err {err:.2e} dB")
    assert err <= DB_ATOL, err
    rm = R["checks"]["spectrum"]["c1_rmse"] + R["checks"]["spectrum"]["c2_rmse"]
    assert float(np.max(np.abs(np.asarray(rm, np.float64) - fx["rmse"]))) <= DB_ATOL
    _same_text(text, str(fx["stdout"]))
    assert os.path.getsize(a["out_csv"]) > 0 and os.path.getsize(a["out_png"]) > 0


@pytest.mark.parametrize("name", [c["name"] for c in vc.L1_CASES])
def test_l1_simulate_gate(name):
    """simulate_gate on its own, up-delay 0 and 250 ms (in samples, on the padded
    frame starts)."""
    torch, A, _, l1 = _mods()
    c = vc.BY_NAME[name]
    x, _, _ = vc.make_pair(c)
    want, starts = vr.frame_levels(x, c["n_fft"], c["hop"])
    for ms in (0, 250.0):
        states, levels = l1.simulate_gate(x, SR, c["n_fft"], c["hop"], vc.T_DBFS, vc.HYST, ms)
        assert np.array_equal(np.asarray(levels), want)
        sim = vr.gate(want, starts, vc.T_DBFS + vc.HYST / 2, vc.T_DBFS - vc.HYST / 2,
                      int(ms * SR / 1000))
        assert states == A.state_names(sim)
        assert len(set(states)) == 2


@pytest.mark.parametrize("n_fft,hop,ch", [(4096, 1000, 2), (3000, 700, 1), (256, 100, 2)])
def test_level_grid_with_a_hop_that_does_not_divide_the_padding(n_fft, hop, ch):
    """Frames at k * hop of the padded signal, kept where 0 <= k * hop - n_fft // 2
    < n: levels, padded starts and both gates for (n_fft // 2) % hop != 0."""
    torch, A, v2, l1 = _mods()
    assert (n_fft // 2) % hop != 0
    x = vc.make_x(dict(x="env", seed=320, ch=ch))[:SR * 3 + 13]
    want, starts = vr.frame_levels(x, n_fft, hop)
    levels, got_starts = A.padded_frame_levels(A._dev(x, ch=True), n_fft, hop)
    assert np.array_equal(levels, want) and np.array_equal(got_starts, starts)
    assert np.array_equal(v2.compute_frame_levels(x, SR, n_fft, hop), want)
    states, lv = l1.simulate_gate(x, SR, n_fft, hop, vc.T_DBFS, vc.HYST, 250.0)
    sim = vr.gate(want, starts, vc.T_DBFS + vc.HYST / 2, vc.T_DBFS - vc.HYST / 2, 250 * SR // 1000)
    assert np.array_equal(np.asarray(lv), want) and states == A.state_names(sim)
    assert len(set(states)) == 2


def test_resident_tensors_give_the_arrays_result():
    """verify() on resident cuda tensors, and with two launches instead of the
    fused one, gives the arrays' result."""
    torch, A, v2, _ = _mods()
    c = vc.BY_NAME["verify_v2_st_4096"]
    x, y, _ = vc.make_pair(c)
    a = dict(vc.v2_args(c), out_prefix=None)
    R1, t1 = _run(v2.verify, x, y, SR, **a)
    R2, t2 = _run(v2.verify, torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda(),
                  SR, **a)
    assert t1 == t2 and np.array_equal(R1["c1_db"], R2["c1_db"])
    R3, _ = _run(v2.verify, x, y, SR, fused=False, **a)
    assert np.array_equal(R1["c2_db"], R3["c2_db"]) and R1["ti"] == R3["ti"]


def test_short_output_is_zero_extended():
    """A y shorter than x by at most n_fft // 2 is zero-extended: the last frame
    ends with x, so it crosses the end of y and reads the zeros.  Rows and band
    energies equal the statement's on its own zero-extended pair; verify() fails
    the length line and raises nothing; a y shorter by more raises."""
    torch, A, v2, _ = _mods()
    c = vc.BY_NAME["verify_v2_st_4096"]
    n_fft, hop = c["n_fft"], c["hop"]
    x0, y0, _ = vc.make_pair(c)
    n = n_fft + hop * 60                           # the last frame ends with x
    cut = n_fft // 2 - 7
    x, y = np.ascontiguousarray(x0[:n]), np.ascontiguousarray(y0[:n - cut])
    F = vr.n_inside(n, n_fft, hop)
    assert (F - 1) * hop + n_fft == n and (F - 1) * hop + n_fft > len(y)
    anchor, lo, hi = _bins(n_fft)
    xd, yd = A.pair_on_device(x, y, n_fft // 2)
    assert yd.shape == xd.shape and float(yd[len(y):].abs().max()) == 0.0
    rows, be = A.verify_spectra(xd, yd, n_fft, hop, anchor=anchor, bands=(*lo, *hi))
    rows, be = rows.cpu().numpy().astype(np.float64), be.cpu().numpy().astype(np.float64)
    last = np.array([F - 1])
    r64, X64, Y64 = vr.ratio_rows(x, y, n_fft, hop, *anchor, dtype=np.float64, idx=last)
    r32, _, _ = vr.ratio_rows(x, y, n_fft, hop, *anchor, dtype=np.float32, idx=last)
    ok = (X64 >= 1e-3 * X64.max()) & (Y64 >= 1e-3 * Y64.max())
    e32 = float(np.max(np.abs(r32.astype(np.float64) - r64)[ok] / r64[ok]))
    err = float(np.max(np.abs(rows[-1:] - r64)[ok] / r64[ok]))
    print(f"short y, last frame: rows err {err:.2e} e32 {e32:.2e}")
    assert err <= vr.rule_bound(e32), (err, e32)
    b64 = vr.band_energies(x, y, n_fft, hop, *lo, *hi, dtype=np.float64, idx=last)
    b32 = vr.band_energies(x, y, n_fft, hop, *lo, *hi, dtype=np.float32, idx=last)
    scale = np.repeat([b64[0, :2].max(), b64[0, 2:].max()], 2)
    e32b = float(np.max(np.abs(b32.astype(np.float64) - b64) / scale))
    errb = float(np.max(np.abs(be[-1:] - b64) / scale))
    assert errb <= vr.rule_bound(e32b), (errb, e32b)
    # the zeros are in it: the full-length y gives another last row
    full, _ = A.verify_spectra(xd, A._dev(np.ascontiguousarray(y0[:n]), ch=True), n_fft, hop,
                               anchor=anchor)
    assert float(np.max(np.abs(full[-1].cpu().numpy() - rows[-1]))) > 1e-3
    R, text = _run(v2.verify, x, y, SR, **dict(vc.v2_args(c), out_prefix=None))
    assert R["exit_code"] == 1 and f"(diff=-{cut}) FAIL" in text
    want = vr.run_v2(x, y, SR, vc.v2_args(c))
    assert [R["c1_n"], R["c2_n"]] == [want["c1_n"], want["c2_n"]]
    assert float(np.max(np.abs(R["c1_db"] - want["c1_db"]))) <= DB_ATOL
    assert float(np.max(np.abs(R["c2_db"] - want["c2_db"]))) <= DB_ATOL
    with pytest.raises(ValueError):
        A.pair_on_device(x, y[:n - n_fft // 2 - 1], n_fft // 2)


# ---------------------------------------------------------------------------
# end to end through the package's own CLIs
# ---------------------------------------------------------------------------

def test_cli_end_to_end(tmp_path, monkeypatch):
    torch, A, v2, l1 = _mods()
    from tomatis_audio_processor_amd import audio_io, process_tomatis
    monkeypatch.chdir(tmp_path)
    c = vc.BY_NAME["verify_v2_st_4096"]
    x = vc.make_x(c)
    audio_io.write("in.flac", x, SR, "FLAC")
    gate = ["--gate_mode", "linear", "--gate_ui", "50", "--gate_scale", "1.0", "--gate_offset",
            str(vc.GATE_OFFSET), "--hyst_db", str(vc.HYST), "--up_delay_ms", "0"]

    def tilt(g):
        return ["--c1_low", str(g), "--c1_high", str(-g), "--c2_low", str(-g), "--c2_high", str(g)]

    def written(p):
        return p if os.path.exists(p) else p.replace(".flac", ".wav")

    # +-5 dB with the state CSV, then validate_layer1
    rc, _ = _run(process_tomatis.main, ["-i", "in.flac", "-o", "out5.flac", "--state_csv",
                                        "st.csv"] + gate + tilt(5.0))
    assert rc == 0
    rc, text = _run(l1.main, ["-i", "in.flac", "-o", written("out5.flac"), "--state_csv", "st.csv",
                              "--gate_offset", str(vc.GATE_OFFSET)])
    assert rc == 0 and "Layer1 验证: PASS" in text, text
    assert os.path.getsize("layer1_spectrum_check.csv") > 0
    assert os.path.getsize("layer1_spectrum_check.png") > 0

    # +-15 dB, then verify_tomatis_15db_v2
    rc, _ = _run(process_tomatis.main, ["-i", "in.flac", "-o", "out15.flac"] + gate + tilt(15.0))
    assert rc == 0
    out15 = written("out15.flac")
    rc, text = _run(v2.main, ["-i", "in.flac", "-o", out15, "--out_prefix", "acc"])
    assert rc == 0 and "验证结果: PASS" in text, text
    for suffix in ("_spectrum.csv", "_spectrum.png", "_tilt_index.png", "_report.txt"):
        assert os.path.getsize("acc" + suffix) > 0
    assert "总体结果: PASS" in open("acc_report.txt", encoding="utf-8").read()

    # the same output with a DC offset, and one sample short: exit 1 on that line
    y, _ = audio_io.read(out15)
    audio_io.write("dc.flac", y + np.float32(0.002), SR, "FLAC")
    rc, text = _run(v2.main, ["-i", "in.flac", "-o", "dc.flac", "--out_prefix", "dc"])
    assert rc == 1 and re.search(r"DC偏移: 0\.00\d+ FAIL", text) and "验证结果: FAIL" in text
    audio_io.write("short.flac", y[:-1], SR, "FLAC")
    rc, text = _run(v2.main, ["-i", "in.flac", "-o", "short.flac", "--out_prefix", "short"])
    assert rc == 1 and "(diff=-1) FAIL" in text and "验证结果: FAIL" in text
    assert "总体结果: FAIL" in open("short_report.txt", encoding="utf-8").read()
