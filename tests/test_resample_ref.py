"""CPU: the numpy statement of the audio resampler (tests/resample_ref.py) is
``scipy.signal.resample_poly``, ``resample.taps`` is scipy's filter for float32
input, and the tile plan of ``resample.outputs_per_workgroup`` fits its LDS."""
import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import resample_ref as rs

RATIOS = [(160, 147), (80, 147), (1, 2), (3, 2), (2, 1), (320, 147), (1, 4)]
ALL_RATIOS = RATIOS + [(40, 147), (6, 1), (3, 1), (512, 511), (1, 8)]
ALL_RATIOS += [(4, 7), (2, 3)]   # K = 36 and K = 31: K mod 4 of 0 and 3


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [1, 23, 1000, 4411])
@pytest.mark.parametrize("up,down", RATIOS)
def test_statement_is_resample_poly(up, down, n, ch):
    x = rs.white(4200 + up + down, 4411, 2)[:n, :ch].astype(np.float64)
    h = rs.taps_unscaled(up, down)
    want = resample_poly(x, up, down, axis=0, window=h)
    got = rs.resample_direct(x, up, down, h * up, np.float64)
    assert got.shape == want.shape == (-(-n * up // down), ch)
    peak = float(np.max(np.abs(want)))
    assert float(np.max(np.abs(got - want))) <= 1e-12 * peak


@pytest.mark.parametrize("n", [1, 23, 1000])
@pytest.mark.parametrize("up,down", [(512, 511), (1, 8), (4, 7), (2, 3)])
def test_scipy64_is_the_statement(up, down, n):
    """``rs.resample_scipy64``, which stands in for the statement at the long
    lengths of tests/test_gpu_resample_paths.py, is the statement."""
    x = rs.white(4300 + up + down, 1000, 8)[:n]
    want = rs.resample_scipy64(x, up, down)
    got = rs.resample_direct(x, up, down, rs.taps(up, down), np.float64)
    assert got.shape == want.shape == (-(-n * up // down), 8)
    peak = float(np.max(np.abs(want)))
    assert peak > 0.0
    assert float(np.max(np.abs(got - want))) <= 1e-12 * peak


def test_tapless_phases():
    h = rs.random_taps(1, 3)
    x = rs.white(4400, 50, 1)[:, 0]
    y = rs.resample_direct(x, 5, 3, h, np.float64)
    mask = rs.tapless(len(y), 5, 3, 3)
    assert mask.any() and not mask.all()
    assert not np.any(y[mask]) and np.all(y[~mask][1:-1] != 0.0)
    assert not rs.tapless(40, 2, 3, 15).any()


@pytest.mark.parametrize("up,down", ALL_RATIOS)
def test_taps_are_scipys_for_float32(up, down):
    from tomatis_audio_processor_amd import resample
    h = resample.taps(up, down)
    assert h.dtype == np.float32 and len(h) == 20 * max(up, down) + 1
    assert np.array_equal(h.view(np.uint32), rs.taps(up, down).view(np.uint32))
    # what scipy applies to float32 input: an impulse long enough to show every tap
    n = -(-len(h) // up) + 2
    x = np.zeros(n, np.float32)
    x[n // 2] = 1.0
    y = resample_poly(x, up, down)
    assert y.dtype == np.float32
    want = rs.impulse_response(n, up, down, h, n // 2)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("ch", [1, 2, 5, 8])
@pytest.mark.parametrize("up,down", ALL_RATIOS)
def test_outputs_per_workgroup_fits(up, down, ch):
    from tomatis_audio_processor_amd import resample
    T = resample.outputs_per_workgroup(up, down, ch)
    assert T >= 1 and T & (T - 1) == 0 and T <= 1024
    n_taps = 20 * max(up, down) + 1
    K = -(-n_taps // up)
    K4 = -(-K // 4) * 4
    # the frames a tile of T outputs reads, whatever its first phase is, up to
    # three words of alignment in front, and one row of >= K4 taps per phase
    span = max((p0 + down * (T - 1)) // up for p0 in range(up)) + K4
    words = resample.lds_words(up, down, ch)
    assert 4 * words <= 64 * 1024
    assert words >= 3 + span * ch + up * K4
    if T < 1024:  # the next size does not fit
        span2 = (up - 1 + down * (2 * T - 1)) // up + K4
        Ks = 4 * ((K4 // 4) | 1)   # rows of an odd number of 16-byte slots
        assert 4 * ((3 + span2 * ch + 3) // 4 * 4 + up * Ks) > 64 * 1024


def test_limits():
    from tomatis_audio_processor_amd import resample
    for sr in (44100, 88200, 176400, 96000, 192000, 32000, 24000, 22050, 16000, 8000, 48000):
        assert resample.supported(sr, 48000), sr
    assert resample.ratio(44100, 48000) == (160, 147)
    assert not resample.supported(48000, 5000)       # 5 / 48: down > 8 up
    assert not resample.supported(48000, 44101)      # max(up, down) > 512
    assert resample.n_out(4411, 160, 147) == len(resample_poly(np.zeros(4411), 160, 147))
