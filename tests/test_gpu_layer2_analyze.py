"""GPU: the layer-2 analysis CLI (workflow step 5) against
the output of the reference's own src/layer2_analyze_eq.py on the same 40 s
pairs (tests/golden/align_cli_*.npz, tools/make_align_goldens.py).

The delay and the frame counts are text-identical.  delta_db_raw is a
difference of two medians minus the median of such differences: three medians
at the analysis spectra's stated 2e-3 dB, so 6e-3 dB.  delta_db_smooth is a
linear filter of the (1-Lipschitz) clipped raw curve: 6e-3 dB times the l1 norm
of the row of scipy's savgol operator that produced the bin (the centre kernel
inside, the polynomial-fit rows of mode="interp" over the first and last half
window).
"""
import functools
import os
import re

import numpy as np
import pytest
from scipy.signal import savgol_coeffs

from tests import align_ref as ar
from tests.golden.align_cases import CLI_CASES, ERROR_CASES, SR, make_pair

pytestmark = pytest.mark.gpu
RAW_ATOL = 3 * 2e-3   # dB


@pytest.fixture(scope="module")
def l2():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, layer2_analyze_eq
    _lib.lib()
    return layer2_analyze_eq


@functools.lru_cache(maxsize=None)
def _pair(seed, n_base, n_target, shift):
    return make_pair(dict(seed=seed, n_base=n_base, n_target=n_target, shift=shift))


def _files(c, tmp_path):
    from tomatis_audio_processor_amd import audio_io
    xt, xb = _pair(c["seed"], c["n_base"], c["n_target"], c["shift"])
    pt, pb = str(tmp_path / "target.wav"), str(tmp_path / "base.wav")
    audio_io.write(pt, xt, SR, "WAV", "FLOAT")
    audio_io.write(pb, xb, SR, "WAV", "FLOAT")
    return pt, pb


def _lines(text, tag):
    return [ln for ln in text.splitlines() if ln.startswith(tag)]


def _savgol_row_norms(n_bins, smooth_bins):
    """l1 norm of every row of savgol_filter(., w, 3, mode="interp") as a matrix."""
    w = int(smooth_bins)
    if w % 2 == 0:
        w += 1
    w = max(11, w)
    if w >= n_bins:
        w = n_bins - 1 if (n_bins - 1) % 2 == 1 else n_bins - 2
    half = w // 2
    norms = np.full(n_bins, float(np.abs(savgol_coeffs(w, 3)).sum()))
    for i in range(half):
        edge = float(np.abs(savgol_coeffs(w, 3, pos=i, use="dot")).sum())
        norms[i] = norms[n_bins - 1 - i] = edge
    return norms


@pytest.mark.parametrize("c", CLI_CASES, ids=lambda c: c["name"])
def test_cli_matches_reference(l2, c, tmp_path, capsys):
    fx = ar.fixture(c["name"])
    pt, pb = _files(c, tmp_path)
    csv, png = str(tmp_path / "curve.csv"), str(tmp_path / "curve.png")
    l2.main(["--base", pb, "--target", pt, "--out_csv", csv, "--out_png", png] + c["argv"])
    out = capsys.readouterr().out
    ref = str(fx["stdout"])
    for tag in ("[ALIGN]", "[STATS]"):
        assert _lines(out, tag) == _lines(ref, tag) and len(_lines(out, tag)) == 1
    assert _lines(out, "[SAVED]") == [f"[SAVED] {csv}", f"[SAVED] {png}"]
    with open(csv) as f:
        assert f.readline().strip() == "freq_hz,delta_db_raw,delta_db_smooth"
    cols = np.loadtxt(csv, delimiter=",", skiprows=1)
    assert np.array_equal(cols[:, 0], fx["freqs"])
    e_raw = float(np.max(np.abs(cols[:, 1] - fx["delta_raw"])))
    smooth_bins = int(c["argv"][c["argv"].index("--smooth_bins") + 1]) \
        if "--smooth_bins" in c["argv"] else 71
    norms = _savgol_row_norms(len(cols), smooth_bins)
    e_s = np.abs(cols[:, 2] - fx["delta_smooth"])
    print(f"CSV {c['name']}: raw {e_raw:.2e} dB, smooth {float(e_s.max()):.2e} dB, "
          f"norms {norms.min():.2f}..{norms.max():.2f}")
    assert e_raw <= RAW_ATOL
    assert np.all(e_s <= RAW_ATOL * norms)
    # the anchor, to the two decimals it is printed with
    pat = re.compile(r"= ([+-]\d+\.\d\d) dB \(removed\)")
    assert _lines(out, "[INFO]")[0].split("=")[0] == _lines(ref, "[INFO]")[0].split("=")[0]
    assert pat.search(out).group(1) == pat.search(ref).group(1)
    assert os.path.getsize(png) > 0


def test_analyze_returns_what_main_prints(l2):
    c = CLI_CASES[1]
    fx = ar.fixture(c["name"])
    xt, xb = _pair(c["seed"], c["n_base"], c["n_target"], c["shift"])
    freqs, d0, ds, anchor, used_b, used_t, delay = l2.analyze(
        xb, xt, n_fft=2048, hop=1024, smooth_bins=31, clamp_db=6.0, log=lambda *a: None)
    assert delay == int(fx["delay"]) and [used_b, used_t] == fx["used"].tolist()
    assert np.array_equal(freqs, fx["freqs"])
    assert d0.dtype == ds.dtype == np.float32 and np.all(np.abs(d0) <= 6.0)
    assert float(np.max(np.abs(d0 - fx["delta_raw"]))) <= RAW_ATOL


@pytest.mark.parametrize("c", ERROR_CASES, ids=lambda c: c["name"])
def test_reference_error_paths(l2, c, tmp_path):
    fx = ar.fixture(c["name"])
    pt, pb = _files(c, tmp_path)
    with pytest.raises(ValueError) as ei:
        l2.main(["--base", pb, "--target", pt, "--out_csv", str(tmp_path / "c.csv"),
                 "--out_png", str(tmp_path / "c.png")] + c["argv"])
    assert str(ei.value) == str(fx["error"])
    assert not os.path.exists(tmp_path / "c.csv")
