"""GPU: the alignment kernels (tm_align.hip) one entry point
at a time and as ``align.find_delay`` against the reference's goldens.

Envelope and correlation are judged like the transforms
(tests/test_gpu_spectral_fidelity.py): with the float64 numpy / scipy statement
y64 of the same operation (tests/align_ref.py) and scipy's own float32 result
y32 of it,

    e = max |y - y64| / max |y64|  <=  8 * max(e32, 2^-23),  e32 = the same of y32.

find_delay is compared as an integer: the test first shows on the CPU that the
float64 correlation's top stands (top - runner-up) / top >= 1e-3 clear on every
case, four orders above float32 rounding of the correlation.

Largest measured e / max(e32, 2^-23) on the MI355X: envelope 0.61 (len 481,
down 6; 0.27 at 240017 samples, down 24), correlation 2.08 (nb 257, 301
outputs; 1.09 at nb 4000, 20001 outputs).
"""
import functools

import numpy as np
import pytest
from scipy.signal import fftconvolve

from tests import align_ref as ar
from tests.golden.align_cases import DELAY_CASES, SR, make_pair
from tests.golden.envelope_bits_cases import BITS_CASES, FIXTURE, make_input, run_entry_point
from tests.stft_ref import white

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, align
    _lib.lib()
    return align


def _rel(y, y64):
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64)) / np.max(np.abs(y64)))


# ---------------------------------------------------------------------------
# envelope
# ---------------------------------------------------------------------------

def _judge_envelope(al, x, down, start, stop, name, ds_sr=None):
    """x[start:stop] through the device against resample_poly; the whole x is
    resident, so the samples around the range are live.  ``ds_sr``: for a
    ``down`` that does not divide 48000."""
    import torch
    sr, ds_sr = (48000, 48000 // down) if ds_sr is None else (down * ds_sr, ds_sr)
    seg = x[start:stop]
    y64, mean64 = ar.envelope(seg, sr, ds_sr, np.float64)     # centred, and its mean
    peak = float(np.max(np.abs(y64 + mean64)))                # of the decimator's output
    y32, mean32 = ar.envelope(seg, sr, ds_sr, np.float32)
    e32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    got, mean = al.envelope_ds(torch.from_numpy(x).cuda(), sr, ds_sr, start, stop, with_mean=True)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == y64.shape
    e = float(np.max(np.abs(got.astype(np.float64) - y64)) / peak)
    print(f"RATIO [envelope] {name}: e {e:.3e} e32 {e32:.3e} ratio {e / max(e32, ar.FLOOR):.2f}")
    assert e <= ar.bound(e32), (name, e, e32)
    assert abs(mean - float(mean32)) <= 2.0 ** -20 * peak, (name, mean, float(mean32))
    return got


@pytest.mark.parametrize("down", [24, 6])
@pytest.mark.parametrize("n", [1, 23, 24, 25, 481, 5 * 48000 + 17])
def test_envelope_against_resample_poly(al, n, down):
    x = white(2000 + n % 1000 + down, n, 2)
    _judge_envelope(al, x, down, 0, n, f"len {n} down {down}")


@pytest.mark.parametrize("down", [24, 6])
def test_envelope_subrange_is_a_signal_of_its_own(al, down):
    """start > 0 with live samples on both sides: they count as zeros."""
    x = white(2100 + down, 9000, 2)
    got = _judge_envelope(al, x, down, 1237, 7001, f"sub-range down {down}")
    # and the host-array form uploads the range alone: the same bits
    host = al.envelope_ds(x, 48000, 48000 // down, 1237, 7001).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


def test_envelope_rejects_other_ratios(al):
    x = white(2200, 1000, 2)
    with pytest.raises(ValueError):
        al.envelope_ds(x, 44100, 2000)
    with pytest.raises(ValueError):
        al.envelope_ds(x, 48000, 500)   # decimation 96 > 64


@functools.lru_cache(maxsize=None)
def _bits_fixture():
    return ar.fixture(FIXTURE)


@pytest.mark.parametrize("case", BITS_CASES, ids=[c["key"] for c in BITS_CASES])
def test_envelope_ds_bits_are_the_parent_commits(al, case):
    """One decimating kernel serves every entry point.  Up to down = 53 it gives
    one thread per output and sums in the order of the integer decimator it
    replaced: the bits and the mean that decimator's library wrote
    (tools/make_envelope_bits_goldens.py), from the C entry point and from
    ``envelope_ds``."""
    import torch
    fx = _bits_fixture()
    key = case["key"]
    x, crc = make_input(case)
    assert crc == int(fx[key + "_crc"]), \
        f"{key}: the input differs from the fixture's (CRC {crc:08x}, not " \
        f"{int(fx[key + '_crc']):08x}): numpy's generator changed, not the kernel"
    bits, mean = run_entry_point(case, x)
    assert np.array_equal(bits, fx[key + "_bits"]), key
    assert mean == float(fx[key + "_mean"]), key
    down = case["down"]
    got, mean = al.envelope_ds(torch.from_numpy(x).cuda(), 1000 * down, 1000, case["start"],
                               case["stop"], with_mean=True, mean_first=case["mean_first"])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), fx[key + "_bits"]), key
    assert mean == float(fx[key + "_mean"]), key


@pytest.mark.parametrize("mean_first", [False, True], ids=["mean-last", "mean-first"])
@pytest.mark.parametrize("per_down,plus", [(0, 1), (0, 65), (600, 17)])
@pytest.mark.parametrize("down", [54, 64])
def test_envelope_two_threads_per_output(al, down, per_down, plus, mean_first):
    """down 54..64: the staging of 256 outputs no longer fits the LDS, a
    workgroup owns 128 outputs with two threads each and the two partial sums
    are added last, so these are not the integer decimator's bits; the bound
    against float64 is the same.  Measured e / max(e32, 2^-23) on the MI355X
    (profiles/align/gpu_tests_one_decimator.log), mean-last / mean-first:
    down 54: 0.53 / 0.87 at 65 frames, 0.13 / 0.28 at 32 417;
    down 64: 0.81 / 1.12 at 65 frames, 0.13 / 0.37 at 38 417; 0.00 at one frame.

    One frame in mean-first order is exact zeros in every precision (the sample
    less its own mean), which leaves the judge no scale to divide by: zeros and
    the mean are asserted instead."""
    from tests.test_gpu_compare import _judge_mean_first
    n = per_down * down + plus
    x = white(2300 + n % 1000 + down, n, 2)
    name = f"len {n} down {down}"
    if not mean_first:
        _judge_envelope(al, x, down, 0, n, name, ds_sr=1000)
    elif n > 1:
        _judge_mean_first(al, x, down, 0, n, name, ds_sr=1000)
    else:
        got, mean = al.envelope_ds(x, 1000 * down, 1000, with_mean=True, mean_first=True)
        assert got.shape == (1,) and not np.any(got.cpu().numpy())
        assert mean == float(ar.power_mono(x)[0])


# ---------------------------------------------------------------------------
# correlation
# ---------------------------------------------------------------------------

XC_NB = [1, 63, 64, 65, 4000]
XC_EXTRA = [0, 1, 2047, 20000]
# a template of exactly one LDS block (1024) over more than one workgroup's
# outputs (4096), one block and a ragged second one, the sub-sum edge (256 + 1)
XC_MORE = [(1024, 4097), (1500, 5000), (257, 300)]


@pytest.mark.parametrize("nb,extra", [(nb, ex) for nb in XC_NB for ex in XC_EXTRA] + XC_MORE)
def test_xcorr_against_float64(al, nb, extra):
    rng = np.random.default_rng(3000 + 31 * nb + extra)
    nt = nb + extra
    b = rng.standard_normal(nb).astype(np.float32)
    t = (0.5 * rng.standard_normal(nt)).astype(np.float32)
    off = extra // 3
    t[off:off + nb] += b          # a coherent peak at off
    c64 = np.correlate(t.astype(np.float64), b.astype(np.float64), mode="valid")
    c32 = fftconvolve(t, b[::-1], mode="valid")
    assert c32.dtype == np.float32
    e32 = _rel(c32, c64)
    got = al.xcorr_valid(t, b).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == c64.shape == (extra + 1,)
    e = _rel(got, c64)
    print(f"RATIO [xcorr] nb {nb} nt-nb {extra}: e {e:.3e} e32 {e32:.3e} "
          f"ratio {e / max(e32, ar.FLOOR):.2f}")
    assert e <= ar.bound(e32), (nb, extra, e, e32)
    again = al.xcorr_valid(t, b).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "run-to-run"


def test_xcorr_needs_nt_ge_nb(al):
    with pytest.raises(ValueError):
        al.xcorr_valid(np.zeros(3, np.float32), np.zeros(4, np.float32))


# ---------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------

def _arg_cases():
    n = 100000                      # 391 workgroups of 256
    rng = np.random.default_rng(4000)
    base = rng.standard_normal(n).astype(np.float32)
    a = base.copy(); a[0] = 9.0
    b = base.copy(); b[n - 1] = 9.0
    c = base.copy(); c[70000] = 9.0; c[300] = 9.0          # two workgroups apart
    d = np.full(n, 2.5, np.float32)
    e = -np.abs(base) - 1.0; e[51234] = -0.5               # all negative
    f = np.zeros(n, np.float32); f[5] = -0.0; f[3] = 0.0   # -0 == +0
    return dict(first=(a, 0), last=(b, n - 1), tie_two_groups=(c, 300), all_equal=(d, 0),
                negative=(e, 51234), zeros=(f, 0), one=(np.array([-3.0], np.float32), 0))


@pytest.mark.parametrize("name", list(_arg_cases()))
def test_argmax_lowest_index_wins(al, name):
    c, want = _arg_cases()[name]
    assert int(np.argmax(c)) == want
    k, v = al.argmax_first(c, with_value=True)
    assert (k, v) == (want, float(c[want]))
    assert al.argmax_first(c, with_value=True) == (k, v), "run-to-run"


# ---------------------------------------------------------------------------
# find_delay against the reference's goldens
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    c = next(c for c in DELAY_CASES if c["name"] == name)
    xt, xb = make_pair(c)
    return c, xt, xb


@pytest.mark.parametrize("name", [c["name"] for c in DELAY_CASES])
def test_find_delay_equals_reference(al, name):
    c, xt, xb = _case(name)
    fx = ar.fixture(name)
    # the condition on the inputs (CPU, float64): the top stands clear
    st64 = ar.delay_estimate(xt, xb, SR, 2000, c["chunk_sec"], np.float64)
    m = ar.margin(st64["corr"])
    print(f"MARGIN {name}: {m:.2e}")
    assert m >= 1e-3, (name, m)
    assert st64["delay"] == int(fx["delay"])
    assert al.find_delay(xt, xb, sr=SR, chunk_sec=c["chunk_sec"]) == int(fx["delay"])


def test_find_delay_takes_resident_tensors_and_paths(al, tmp_path):
    import torch
    from tomatis_audio_processor_amd import audio_io
    c, xt, xb = _case("align_p1234")
    want = int(ar.fixture(c["name"])["delay"])
    dt, db = torch.from_numpy(np.array(xt)).cuda(), torch.from_numpy(np.array(xb)).cuda()
    assert al.find_delay(dt, db, sr=SR, chunk_sec=c["chunk_sec"]) == want
    pt, pb = str(tmp_path / "t.wav"), str(tmp_path / "b.wav")
    audio_io.write(pt, xt, SR, "WAV", "FLOAT")
    audio_io.write(pb, xb, SR, "WAV", "FLOAT")
    assert al.find_delay(pt, pb, sr=SR, chunk_sec=c["chunk_sec"]) == want
    with pytest.raises(AssertionError):
        al.find_delay(pt, pb, sr=44100)


def test_host_fallback_cases(al):
    """The target's envelope shorter than the base chunk's, and up != 1: the
    host scipy body, the same integer as the device path where both apply."""
    c, xt, xb = _case("align_short_target")
    assert -(-len(xt) // 24) < 4000
    assert al.find_delay(xt, xb, sr=SR, chunk_sec=2) == int(ar.fixture(c["name"])["delay"])
    c, xt, xb = _case("align_m5000")
    assert al._find_delay_host(xt, xb, SR, 2000, 2) == al.find_delay(xt, xb, sr=SR, chunk_sec=2)
    assert not al.device_ratio(48000, 1800)
    st = ar.delay_estimate(xt, xb, SR, 1800, 2)
    assert al.find_delay(xt, xb, sr=SR, ds_sr=1800, chunk_sec=2) == st["delay"]
