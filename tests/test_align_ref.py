"""Alignment and layer-2 analysis on the CPU: the numpy
statement tests/align_ref.py against the goldens made by the reference's own
src/layer2_analyze_eq.py (tools/make_align_goldens.py), the formula the device
decimator implements against scipy's resample_poly, and the package's
bins-sized tail (anchor, clip, savgol) against the golden CSV columns."""
import json

import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import align_ref as ar
from tests.golden.align_cases import CLI_CASES, DELAY_CASES, SR, make_pair
from tests.golden_util import sha
from tests.stft_ref import white


def _pair(c, fx):
    xt, xb = make_pair(c)
    assert [sha(xt), sha(xb)] == [str(s) for s in fx["in_sha"]], "input generator drifted"
    assert json.loads(str(fx["meta"])) == c
    return xt, xb


@pytest.mark.parametrize("c", DELAY_CASES + CLI_CASES, ids=lambda c: c["name"])
def test_statement_reproduces_golden_k_and_delay(c):
    fx = ar.fixture(c["name"])
    xt, xb = _pair(c, fx)
    st = ar.delay_estimate(xt, xb, SR, 2000, c.get("chunk_sec", 25.0))
    assert st["k"] == int(fx["k"])
    assert st["delay"] == int(fx["delay"])


@pytest.mark.parametrize("c", DELAY_CASES, ids=lambda c: c["name"])
def test_golden_margins(c):
    """The inputs' condition for integer equality of a float32 delay: the
    float64 correlation's top stands clear of its runner-up."""
    assert float(ar.fixture(c["name"])["margin64"]) >= 1e-3


@pytest.mark.parametrize("down", [24, 6])
@pytest.mark.parametrize("n", [1, 23, 24, 25, 481, 4817])
def test_decimator_formula_is_resample_poly(n, down):
    """y[j] = sum_m h[m] e[down j + 10 down - m], j < ceil(n / down), with
    resample_poly's float32 filter, in float64 against resample_poly on the
    float32 envelope.  The bound is the worst case of a float32 dot product of
    n_taps terms (Higham: n u sum |h| |e|, u = 2^-24; two more roundings for the
    float32 envelope itself); a misplaced tap or phase is O(1)."""
    from scipy.signal import firwin
    x = white(7000 + n + down, n, 2)
    e32 = ar.power_mono(x)
    got = resample_poly(e32, 1, down)
    assert got.dtype == np.float32
    want = ar.envelope_direct(x, down, np.float64)
    assert got.shape == want.shape == (-(-n // down),)
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0)).astype(np.float32)
    tol = (len(h) + 2) * 2.0 ** -24 * float(np.abs(h).sum()) * float(e32.max())
    assert float(np.max(np.abs(got - want))) <= tol


def _tail_args(argv):
    kw = dict(anchor_lo=300.0, anchor_hi=3000.0, clamp_db=12.0, smooth_bins=71)
    for k, v in zip(argv[0::2], argv[1::2]):
        if k[2:] in kw:
            kw[k[2:]] = type(kw[k[2:]])(v)
    return kw


@pytest.mark.parametrize("c", CLI_CASES, ids=lambda c: c["name"])
def test_tail_reproduces_golden_csv(c):
    from tomatis_audio_processor_amd import layer2_analyze_eq as l2
    fx = ar.fixture(c["name"])
    d0, ds, anchor = l2.eq_tail(fx["freqs"], fx["med_b"], fx["med_t"], **_tail_args(c["argv"]))
    assert d0.dtype == ds.dtype == np.float32
    assert np.array_equal(d0.astype(np.float64), fx["delta_raw"])
    assert np.array_equal(ds.astype(np.float64), fx["delta_smooth"])
    assert f"= {anchor:+.2f} dB (removed)" in str(fx["stdout"])
