"""The rational-ratio decimator on the CPU: the formula the device implements
(tests/rational_ref.py) against scipy's resample_poly, the goldens made by the
reference's two delay estimates at 44.1, 88.2 and 192 kHz
(tools/make_rational_goldens.py) against the numpy statements, and the
binding of the new entry point."""
import ctypes
import json

import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import align_ref as ar
from tests import compare_ref as cr
from tests import rational_ref as rr
from tests.golden.rational_cases import DS_SR, MIN_MARGIN, RATIONAL_CASES
from tests.golden_util import sha
from tests.stft_ref import white

RATIOS = [(20, 441), (10, 441), (5, 441), (1, 96), (3, 80)]


def _lengths(down):
    return [1, 23, down - 1, down, down + 1, 5000]


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "1-D"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_decimator_formula_is_resample_poly(up, down, mono):
    """out[j] = sum_i h[down j + half - up i] e[i] with ``_taps_rational``'s
    filter, in float64, against resample_poly on the float32 envelope.  The
    bound is the one of tests/test_align_ref.py: the worst case of a float32
    dot product of n_taps terms (Higham: n u sum |h| |e|, u = 2^-24; two more
    roundings for the float32 envelope itself); a misplaced tap or phase is O(1)."""
    from tomatis_audio_processor_amd import align
    h = align._taps_rational(up, down)
    assert h.dtype == np.float32 and h.shape == (20 * down + 1,)
    assert np.array_equal(h, rr.taps(up, down))
    for n in _lengths(down):
        x = white(9000 + n + down + up, n, 2)
        e32 = rr.envelope_of(x[:, 0] if mono else x)
        assert e32.dtype == np.float32 and e32.shape == (n,)
        got = resample_poly(e32, up, down)
        assert got.dtype == np.float32
        want = rr.resample_direct(e32, up, down, h)
        assert got.shape == want.shape == (-(-n * up // down),)
        tol = (len(h) + 2) * 2.0 ** -24 * float(np.abs(h).sum()) * float(np.abs(e32).max())
        err = float(np.max(np.abs(got - want)))
        assert err <= tol, (up, down, n, err, tol)


def test_ratio_predicates():
    from tomatis_audio_processor_amd import align
    for sr, ud in [(44100, (20, 441)), (88200, (10, 441)), (176400, (5, 441)), (192000, (1, 96))]:
        assert align._ratio(sr, DS_SR) == rr.ratio(sr, DS_SR) == ud
        assert align.rational_ratio(sr, DS_SR) and not align.device_ratio(sr, DS_SR)
    assert align.rational_ratio(48000, 1800) and not align.device_ratio(48000, 1800)   # 3 / 80
    assert align.rational_ratio(48000, 2000) and align.device_ratio(48000, 2000)       # both
    assert not align.rational_ratio(1000, 2000)        # up > down
    assert not align.rational_ratio(2000, 2000)
    assert not align.rational_ratio(2000 * 513, 2000)  # down 513
    assert not align.rational_ratio(131 * 67, 65 * 67)  # 65 / 131: up > 64


def _fixture(c):
    fx = ar.fixture(c["name"])
    _, xt, xb = rr.pair(c["name"])
    assert [sha(xt), sha(xb)] == [str(s) for s in fx["in_sha"]], "input generator drifted"
    assert json.loads(str(fx["meta"])) == c
    return fx, xt, xb


@pytest.mark.parametrize("c", RATIONAL_CASES, ids=lambda c: c["name"])
def test_statements_reproduce_golden_k_and_delay(c):
    fx, xt, xb = _fixture(c)
    st = ar.delay_estimate(xt, xb, c["sr"], DS_SR, c["chunk_sec"])
    assert (st["k"], st["delay"]) == (int(fx["k"]), int(fx["delay"]))
    sf = cr.delay_estimate(xb, xt, c["sr"], DS_SR)
    assert (sf["k"], sf["nb"], sf["delay"]) == (int(fx["k_full"]), int(fx["nb"]),
                                                int(fx["delay_full"]))
    # both estimates land within one envelope sample of the shift the pair was cut with
    step = c["sr"] / DS_SR
    assert abs(int(fx["delay"]) - c["shift"]) <= 1.5 * step
    assert abs(int(fx["delay_full"]) - c["shift"]) <= 1.5 * step


@pytest.mark.parametrize("c", RATIONAL_CASES, ids=lambda c: c["name"])
def test_golden_margins(c):
    fx = ar.fixture(c["name"])
    assert float(fx["margin64"]) >= MIN_MARGIN
    assert float(fx["margin64_full"]) >= MIN_MARGIN


def test_new_entry_point_is_bound_and_exported():
    from tomatis_audio_processor_amd import _lib
    name = "tomatis_align_envelope_rational"
    assert name in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    assert (_lib.E_ARG, _lib.E_UNSUPPORTED) == (-1, -2)
