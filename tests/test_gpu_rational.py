"""GPU: the decimator at rational ratios (tm_align.hip k_al_envelope behind
``tomatis_align_envelope_rational``) on its own, and ``align.find_delay`` /
``find_delay_full`` / ``compare_audio.find_delay_by_corr`` at 44.1, 88.2 and
192 kHz against the reference's goldens (tools/make_rational_goldens.py).

The envelope is judged like the integer decimator's (tests/test_gpu_align.py):
with the float64 statement y64 of the operation (tests/rational_ref.py) and
scipy's own float32 result y32 of it, relative to the decimator's output peak,

    e = max |y - y64| / peak  <=  8 * max(e32, 2^-23),  e32 = the same of y32.

Delays are compared as integers after the stored float64 margin of the
correlation's top is shown to be >= 1e-3; the delay tests patch the host
scipy bodies to raise, so the device did the work.

Shapes: one sample, fewer than one output's span, down -+ 1, exactly T and
T + 1 outputs (T: the outputs of one workgroup, ``rational_ref.
outputs_per_workgroup``), and 5 s + 17 samples at 44.1 kHz (10 001 outputs,
40 workgroups, every one of the 20 tap phases).

Largest measured e / max(e32, 2^-23) on the MI355X: 1.48 (2 / 511 mean-first,
512 samples), 1.41 (1 / 96 mean-first, 97 samples); 0.73 at 20 / 441; 0.27 at
220 517 samples.  1 / 24 returns the bits of ``envelope_ds``: the same kernel
behind another range check (tests/test_gpu_align.py pins those bits).
"""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import align_ref as ar
from tests import compare_ref as cr
from tests import rational_ref as rr
from tests.golden.rational_cases import DS_SR, MIN_MARGIN, RATIONAL_CASES
from tests.stft_ref import white

pytestmark = pytest.mark.gpu

RATES = {(20, 441): (44100, 2000), (10, 441): (88200, 2000), (5, 441): (176400, 2000),
         (1, 96): (192000, 2000), (3, 80): (48000, 1800), (1, 24): (48000, 2000),
         # the kernel's other paths: up == 1 with the taps read from global memory (T = 64 and,
         # at the largest ratio, T = 8 with 32 threads per output), up > 1 with T = 4
         (1, 160): (320000, 2000), (1, 512): (1024000, 2000), (2, 511): (511000, 2000)}


@pytest.fixture(scope="module")
def al():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, align
    _lib.lib()
    yield align
    rr.pair.cache_clear()   # the 192 kHz pair: nothing is kept for the rest of the suite


@pytest.fixture
def no_host(al, monkeypatch):
    """The host scipy bodies raise: what passes ran on the device."""
    def refuse(*a, **k):
        raise AssertionError("the host body ran")
    for name in ("_find_delay_host", "_find_delay_full_host", "_delay_full_host"):
        monkeypatch.setattr(al, name, refuse)
    return al


def _edge(up, down):
    """The largest n with exactly T outputs."""
    return rr.outputs_per_workgroup(up, down) * down // up


def _shapes(up, down):
    n_t, T = _edge(up, down), rr.outputs_per_workgroup(up, down)
    assert -(-n_t * up // down) == T and -(-(n_t + 1) * up // down) == T + 1
    return [1, 23, down - 1, down + 1, n_t, n_t + 1]


# ---------------------------------------------------------------------------
# the envelope
# ---------------------------------------------------------------------------

def _judge(al, x, up, down, start, stop, mean_first, name, resident=True):
    """x[start:stop] through envelope_rs against the float64 statement; the
    whole x is resident, so the samples around the range are live."""
    import torch
    sr, ds_sr = RATES[(up, down)]
    h = al._taps_rational(up, down)
    seg = x[start:stop]
    y64, mean64 = rr.envelope_rs(seg, up, down, h, mean_first, np.float64)
    e32 = rr.envelope_of(seg, np.float32)
    if mean_first:
        mean32 = e32.mean()
        y32 = resample_poly(e32 - mean32, up, down).astype(np.float32)
        peak = float(np.max(np.abs(y64)))
    else:
        y32 = resample_poly(e32, up, down).astype(np.float32)
        mean32 = np.mean(y32)
        y32 = y32 - mean32
        peak = float(np.max(np.abs(y64 + mean64)))      # of the decimator's output
    src = torch.from_numpy(np.ascontiguousarray(x)).cuda() if resident else x
    got, mean = al.envelope_rs(src, sr, ds_sr, start, stop, with_mean=True, mean_first=mean_first)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == y64.shape == (-(-len(seg) * up // down),)
    order = "mean-first" if mean_first else "mean-last"
    if peak == 0.0:
        # one sample less its own mean: exact zeros in every precision, no scale to divide by
        assert mean_first and len(seg) == 1 and not np.any(y32) and not np.any(got), name
        assert mean == float(e32[0])
        return got
    err32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    e = float(np.max(np.abs(got.astype(np.float64) - y64)) / peak)
    print(f"RATIO [envelope_rs {up}/{down} {order}] {name}: e {e:.3e} e32 {err32:.3e} "
          f"ratio {e / max(err32, ar.FLOOR):.2f}")
    assert e <= ar.bound(err32), (name, e, err32)
    if mean_first:
        # every float32 e[i] is within 2^-23 of its float64 value, so is their mean
        scale = float(np.mean(np.abs(rr.envelope_of(seg, np.float64))))
        assert abs(mean - float(mean64)) <= 2.0 ** -22 * scale, (name, mean, float(mean64))
    else:
        assert abs(mean - float(mean32)) <= 2.0 ** -20 * peak, (name, mean, float(mean32))
    return got


ALL_SHAPES = [(up, down, n) for up, down in [(20, 441), (1, 96)] for n in _shapes(up, down)]
ALL_SHAPES += [(20, 441, 5 * 44100 + 17), (1, 96, 96 * 300 + 5)]
THREE_SHAPES = [(up, down, n) for up, down in [(10, 441), (5, 441), (3, 80), (1, 160), (1, 512),
                                               (2, 511)]
                for n in (down + 1, _edge(up, down) + 1, 3 * _edge(up, down) + 7)]


@pytest.mark.parametrize("mean_first", [False, True], ids=["mean-last", "mean-first"])
@pytest.mark.parametrize("up,down,n", ALL_SHAPES + THREE_SHAPES)
def test_envelope_against_float64(al, up, down, n, mean_first):
    x = white(9100 + n % 1000 + down + up, n, 2)
    got = _judge(al, x, up, down, 0, n, mean_first, f"len {n}")
    again = al.envelope_rs(x, *RATES[(up, down)], mean_first=mean_first).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "run-to-run"


@pytest.mark.parametrize("mean_first", [False, True], ids=["mean-last", "mean-first"])
def test_integer_ratio_agrees_with_the_integer_decimator(al, mean_first):
    """1 / 24 is legal through ``envelope_rs`` too: the same bound against
    float64, and the bits of ``envelope_ds``, which is the same kernel behind
    another range check (one summation order; tests/test_gpu_align.py holds it
    to the bits of the integer decimator it replaced)."""
    n = 5 * 48000 + 17
    x = white(9200, n, 2)
    got = _judge(al, x, 1, 24, 0, n, mean_first, f"len {n}")
    old = al.envelope_ds(x, 48000, 2000, mean_first=mean_first).cpu().numpy()
    h = al._taps_rational(1, 24)
    assert np.array_equal(h, al._taps(24))
    y64, mean64 = rr.envelope_rs(x, 1, 24, h, mean_first, np.float64)
    peak = float(np.max(np.abs(y64 if mean_first else y64 + mean64)))
    e32env = rr.envelope_of(x)
    if mean_first:
        y32 = resample_poly(e32env - e32env.mean(), 1, 24)
    else:
        y32 = resample_poly(e32env, 1, 24)
        y32 = y32 - np.mean(y32)
    e32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    d = float(np.max(np.abs(got.astype(np.float64) - old.astype(np.float64))) / peak)
    print(f"RATIO [envelope_rs 1/24 against envelope_ds]: d {d:.3e} e32 {e32:.3e} "
          f"ratio {d / max(e32, ar.FLOOR):.2f}")
    assert d <= ar.bound(e32), (d, e32)
    assert np.array_equal(got.view(np.uint32), old.view(np.uint32))


@pytest.mark.parametrize("up,down", [(20, 441), (1, 96)])
@pytest.mark.parametrize("mean_first", [False, True], ids=["mean-last", "mean-first"])
def test_subrange_is_a_signal_of_its_own(al, up, down, mean_first):
    """An odd start with live samples on both sides: they count as zeros; the
    host-array form uploads the range alone and gives the same bits."""
    x = white(9300 + down, 30000, 2)
    got = _judge(al, x, up, down, 1237, 27001, mean_first, "sub-range")
    host = al.envelope_rs(x, *RATES[(up, down)], 1237, 27001, mean_first=mean_first).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


def test_stereo_pointer_of_four_byte_alignment(al):
    """A resident stereo buffer that starts on an odd float takes the scalar
    loads: the same bits as the 8-byte path."""
    import torch
    x = white(9400, 12001, 2)
    want = al.envelope_rs(x, 44100, 2000).cpu().numpy()
    flat = torch.zeros(2 * len(x) + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    view = flat[1:].view(len(x), 2)
    assert view.data_ptr() % 8 == 4
    got = al.envelope_rs(view, 44100, 2000).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("up,down", [(20, 441), (1, 96)])
@pytest.mark.parametrize("mean_first", [False, True], ids=["mean-last", "mean-first"])
def test_one_dimensional_input_at_an_odd_start(al, up, down, mean_first):
    """The reference's 1-D power-mono argument (``channels == 1``): used as
    given; the range starts on an odd sample, a pointer of 4-byte alignment."""
    x = white(9500 + down, 30000, 2)
    e = ar.power_mono(x)                                  # float32, positive
    got = _judge(al, e, up, down, 1237, 27001, mean_first, "1-D sub-range")
    host = al.envelope_rs(e, *RATES[(up, down)], 1237, 27001, mean_first=mean_first).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    # and the stereo form of the same signal, power_mono formed on the device: an
    # envelope sample differs by at most an ulp (2^-24 e) from numpy's, the taps of
    # one output sum to about 1 in magnitude (< 2): 2^-23 max e, with room for the
    # float64 means; the FMA order is the same
    st = al.envelope_rs(x, *RATES[(up, down)], 1237, 27001, mean_first=mean_first).cpu().numpy()
    assert float(np.max(np.abs(st - got))) <= 2.0 ** -21 * float(e.max())


def test_envelope_rs_rejects_what_the_kernel_does_not_take(al):
    x = white(9600, 1000, 2)
    with pytest.raises(ValueError):
        al.envelope_rs(x, 1000, 2000)            # up > down
    with pytest.raises(ValueError):
        al.envelope_rs(x, 2000 * 513, 2000)      # down 513
    with pytest.raises(ValueError):
        al.envelope_rs(x, 44100, 2000, 500, 500)  # empty range


def test_abi_refusals_come_before_any_read(al):
    """Each refusal with a buffer of 64 floats behind a claimed 10^9 frames."""
    import torch
    from tomatis_audio_processor_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    mean = torch.zeros(_lib.ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
    big = 10 ** 9

    def call(channels=2, up=20, down=441, n_taps=21, x=buf, taps=buf, out=buf, start=0, ln=big):
        return h.tomatis_align_envelope_rational(
            _lib.ptr(x) if x is not None else C.c_void_p(0), big, start, ln, channels, up, down,
            _lib.ptr(taps) if taps is not None else C.c_void_p(0), n_taps, 0,
            _lib.ptr(out) if out is not None else C.c_void_p(0), _lib.ptr(mean), C.c_void_p(0))

    assert call(up=1, down=513) == _lib.E_UNSUPPORTED
    assert call(up=65, down=66) == _lib.E_UNSUPPORTED
    assert call(up=1, down=24, n_taps=20 * 24 + 3) == _lib.E_UNSUPPORTED
    assert call(up=5, down=5) == _lib.E_ARG
    assert call(up=7, down=3) == _lib.E_ARG
    assert call(up=0, down=3) == _lib.E_ARG
    assert call(n_taps=20) == _lib.E_ARG
    assert call(channels=3) == _lib.E_ARG
    assert call(channels=0) == _lib.E_ARG
    assert call(x=None) == _lib.E_ARG
    assert call(taps=None) == _lib.E_ARG
    assert call(out=None) == _lib.E_ARG
    assert call(start=1) == _lib.E_ARG            # start + len > n_total
    assert call(ln=0) == _lib.E_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# the delay estimates against the reference's goldens
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c["name"] for c in RATIONAL_CASES])
def test_find_delay_equals_reference(no_host, name):
    import torch
    al = no_host
    c, xt, xb = rr.pair(name)
    fx = ar.fixture(name)
    sr = c["sr"]
    print(f"MARGIN {name}: valid {float(fx['margin64']):.2e} full {float(fx['margin64_full']):.2e}")
    assert float(fx["margin64"]) >= MIN_MARGIN and float(fx["margin64_full"]) >= MIN_MARGIN
    assert not al.device_ratio(sr, DS_SR) and al.rational_ratio(sr, DS_SR)
    # layer2_analyze_eq's estimate: arrays, resident tensors
    want = int(fx["delay"])
    assert al.find_delay(xt, xb, sr=sr, chunk_sec=c["chunk_sec"]) == want
    dt, db = torch.from_numpy(np.array(xt)).cuda(), torch.from_numpy(np.array(xb)).cuda()
    assert al.find_delay(dt, db, sr=sr, chunk_sec=c["chunk_sec"]) == want
    s, e = al._chunk(len(xb), sr, c["chunk_sec"])
    mb = al.envelope_rs(db, sr, DS_SR, s, e)
    k = al.argmax_first(al.xcorr_valid(al.envelope_rs(dt, sr, DS_SR), mb))
    assert k == int(fx["k"])                      # the arg-max itself
    # compare_audio's estimate: the target is the candidate
    want = int(fx["delay_full"])
    assert al.find_delay_full(xb, xt, sr=sr) == want
    assert al.find_delay_full(db, dt, sr=sr) == want
    b = al.envelope_rs(db, sr, DS_SR, mean_first=True)
    k = al.argmax_first(al.xcorr_full(al.envelope_rs(dt, sr, DS_SR, mean_first=True), b))
    assert (k, b.numel()) == (int(fx["k_full"]), int(fx["nb"]))


def test_delays_from_wav_paths_and_the_workflow_functions(no_host, tmp_path):
    """Paths at 44.1 kHz through align and through the find_delay_by_corr of the
    three workflow modules, which pass ``sr`` on."""
    from tomatis_audio_processor_amd import audio_io
    from tomatis_audio_processor_amd import calibrate_to_baseline_v2 as cal
    from tomatis_audio_processor_amd import compare_audio as ca
    from tomatis_audio_processor_amd import layer2_analyze_eq as l2
    al = no_host
    c, xt, xb = rr.pair("rational_44100_p1234")
    fx = ar.fixture(c["name"])
    pt, pb = str(tmp_path / "t.wav"), str(tmp_path / "b.wav")
    audio_io.write(pt, xt, 44100, "WAV", "FLOAT")
    audio_io.write(pb, xb, 44100, "WAV", "FLOAT")
    assert al.find_delay(pt, pb, sr=44100, chunk_sec=2) == int(fx["delay"])
    assert l2.find_delay_by_corr(pt, pb, sr=44100, chunk_sec=2) == int(fx["delay"])
    assert cal.find_delay_by_corr(pt, pb, sr=44100, chunk_sec=2) == int(fx["delay"])
    assert al.find_delay_full(pb, pt, sr=44100) == int(fx["delay_full"])
    assert ca.find_delay_by_corr(pb, pt, 44100) == int(fx["delay_full"])
    with pytest.raises(AssertionError):
        al.find_delay(pt, pb, sr=48000)           # the files are at 44.1 kHz


def test_find_delay_by_corr_takes_the_reference_s_1d_arguments(no_host):
    """compare_audio.find_delay_by_corr(power_mono(b), power_mono(c), sr) on the
    device at 44.1 kHz (20 / 441) and at 48 kHz (1 / 24 through the rational
    entry point), arrays and resident tensors."""
    import torch
    from tests.golden.compare_cases import DELAY_CASES_FULL, SR, make_inputs
    from tomatis_audio_processor_amd import compare_audio as ca
    c, xt, xb = rr.pair("rational_44100_p1234")
    want = int(ar.fixture(c["name"])["delay_full"])
    mb, mc = ca.power_mono(xb), ca.power_mono(xt)
    assert mb.ndim == 1 and mb.dtype == np.float32
    assert ca.find_delay_by_corr(mb, mc, 44100) == want
    assert ca.find_delay_by_corr(torch.from_numpy(mb).cuda(), torch.from_numpy(mc).cuda(),
                                 44100) == want
    c48 = DELAY_CASES_FULL[0]
    base, cand = make_inputs(c48)
    fx = cr.fixture(c48["name"])
    assert float(fx["margin64"]) >= MIN_MARGIN
    assert ca.find_delay_by_corr(ca.power_mono(base), ca.power_mono(cand), SR) == int(fx["delay"])


def test_compare_at_44100_reaches_the_device(no_host):
    from tomatis_audio_processor_amd import compare_audio as ca
    c, xt, xb = rr.pair("rational_44100_m5003")
    lines = []
    ret = ca.compare(xb, xt, sr=44100, n_fft=1024, hop=256, log=lines.append)
    want = int(ar.fixture(c["name"])["delay_full"])
    assert ret[2] == want
    assert lines[0].startswith(f"[ALIGN] delay_samples (cand - base) = {want} ")
