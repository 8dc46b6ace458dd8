"""GPU: the audio resampler (tm_resample.hip k_rs_poly behind
``tomatis_resample_poly`` / ``resample.resample_poly``).

1. A unit impulse returns the taps themselves: every output is
   ``taps[down j + half - up (i0 - start)]`` or zero as bits, the other channels
   exactly zero.  No tolerance: a wrong phase, index or interleave shows.
2. White noise against the float64 statement (tests/resample_ref.py), judged as
   the decimator is (tests/test_gpu_rational.py): with y64 the statement and y32
   scipy's own float32 ``resample_poly`` of the same input, relative to the
   output peak,

       e = max |y - y64| / peak  <=  8 * max(e32, 2^-23),  e32 = the same of y32.

   Shapes: 1, 2 and 23 frames, down -+ 1, exactly T and T + 1 outputs (T: the
   output frames of one workgroup, ``resample.outputs_per_workgroup``), three
   tiles + 7 and one second + 17 samples.
3. Bit equalities: run to run, host array against resident tensor, a sub-range
   at an odd start inside a buffer of ones against the range alone (the
   zero-outside rule), a channel of a 2- or 5-channel run against its mono run.
4. The argument guards of the entry point and the ValueErrors of resample.py.

Largest measured e / max(e32, 2^-23) on the MI355X: 0.98 (1 / 8, 7 frames), 0.76
(1 / 4, 3 frames), 0.69 (6 / 1); 0.55 at 160 / 147 (DESIGN.md §7i has every ratio).
"""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import align_ref as ar
from tests import resample_ref as rs

pytestmark = pytest.mark.gpu

# ratio -> the source rate that gives it on the way to 48 kHz (or a made-up pair)
RATES = {(160, 147): 44100, (80, 147): 88200, (40, 147): 176400, (1, 2): 96000, (1, 4): 192000,
         (3, 2): 32000, (2, 1): 24000, (320, 147): 22050, (6, 1): 8000, (3, 1): 16000}
LIMITS = [(512, 511), (1, 8)]


@pytest.fixture(scope="module")
def rsm():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, resample
    _lib.lib()
    yield resample
    rs.white.cache_clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _T(rsm, up, down, ch):
    return rsm.outputs_per_workgroup(up, down, ch)


# ---------------------------------------------------------------------------
# 1. impulses
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 2, 5])
@pytest.mark.parametrize("up,down", [(160, 147), (1, 2), (3, 1)])
def test_impulse_exact(rsm, up, down, ch):
    import torch
    h = rsm.taps(up, down)
    T = _T(rsm, up, down, ch)
    n = rs.edge_len(T, up, down) + rs.edge_len(T, up, down) // 2 + 3   # one tile and a half
    mid = (T // 2 + 5) * down // up                                    # inside the first tile
    for i0 in (0, n - 1, mid, rs.edge_len(T, up, down)):
        for c in sorted({0, ch - 1}):
            x = rs.impulse(n, ch, i0, c)
            y = rsm.resample_poly(x, up, down).cpu().numpy()
            assert y.shape == (-(-n * up // down), ch)
            want = rs.impulse_response(n, up, down, h, i0)
            assert np.any(want), (i0, c)
            assert np.array_equal(_bits(y[:, c]), _bits(want)), (i0, c)
            others = np.delete(y, c, axis=1)
            assert not np.any(_bits(others)), (i0, c)
    # inside a longer resident buffer, at an odd start: i0 counts from the start of the range
    start, i0 = 7, mid
    big = np.zeros((n + 20, ch), np.float32)
    big[start + i0, ch - 1] = 1.0
    y = rsm.resample_poly(torch.from_numpy(big).cuda(), up, down, start, start + n).cpu().numpy()
    want = rs.impulse_response(n, up, down, h, i0)
    assert np.array_equal(_bits(y[:, ch - 1]), _bits(want))


# ---------------------------------------------------------------------------
# 2. against float64
# ---------------------------------------------------------------------------

def _judge(rsm, x, up, down, name):
    h = rsm.taps(up, down)
    y64 = rs.resample_direct(x, up, down, h, np.float64)
    y32 = resample_poly(x, up, down, axis=0)
    assert y32.dtype == np.float32
    got = rsm.resample_poly(x, up, down).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == y64.shape == y32.shape
    peak = float(np.max(np.abs(y64)))
    assert peak > 0.0
    e32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    e = float(np.max(np.abs(got.astype(np.float64) - y64)) / peak)
    print(f"RATIO [resample_poly {up}/{down} ch {x.shape[1]}] {name}: e {e:.3e} e32 {e32:.3e} "
          f"ratio {e / max(e32, ar.FLOOR):.2f}")
    assert e <= ar.bound(e32), (name, e, e32)
    return got


def _lengths(rsm, up, down, ch, sr):
    n_t = rs.edge_len(_T(rsm, up, down, ch), up, down)
    return sorted({1, 2, 23, max(1, down - 1), down + 1, n_t, n_t + 1, 3 * n_t + 7, sr + 17})


CASES = [(u, d, 2) for u, d in list(RATES) + LIMITS if (u, d) != (3, 1)]
CASES += [(160, 147, 1), (160, 147, 5), (1, 2, 1), (1, 2, 5)]


@pytest.mark.parametrize("up,down,ch", CASES)
def test_against_float64(rsm, up, down, ch):
    sr = RATES.get((up, down), 8000)
    lens = _lengths(rsm, up, down, ch, sr)
    src = rs.white(7300 + up + down, max(lens), 5)
    for n in lens:
        _judge(rsm, np.ascontiguousarray(src[:n, :ch]), up, down, f"len {n}")


# ---------------------------------------------------------------------------
# 3. bit equalities
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("up,down", [(160, 147), (1, 2), (3, 2)])
def test_bit_equalities(rsm, up, down):
    import torch
    T = _T(rsm, up, down, 2)
    n = 2 * rs.edge_len(T, up, down) + 11
    x = np.ascontiguousarray(rs.white(8100 + up, n, 5)[:, :2])
    first = rsm.resample_poly(x, up, down).cpu().numpy()
    again = rsm.resample_poly(x, up, down).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(again)), "run to run"
    res = rsm.resample_poly(torch.from_numpy(x).cuda(), up, down).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(res)), "host array / resident tensor"
    # the zero-outside rule: the range at an odd start inside a buffer of ones
    start = 13
    big = np.ones((n + 40, 2), np.float32)
    big[start:start + n] = x
    sub = rsm.resample_poly(torch.from_numpy(big).cuda(), up, down, start, start + n).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(sub)), "sub-range of a live buffer"
    sub_host = rsm.resample_poly(big, up, down, start, start + n).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(sub_host)), "sub-range of a host array"
    # a shorter range of the same samples: the outputs whose K samples lie inside both agree
    K = -(-len(rsm.taps(up, down)) // up)
    cut = n - 101
    short = rsm.resample_poly(x, up, down, 0, cut).cpu().numpy()
    safe = (cut - K - 1) * up // down - 1
    assert np.array_equal(_bits(first[:safe]), _bits(short[:safe])), "independent of len"


@pytest.mark.parametrize("up,down", [(160, 147), (1, 2)])
def test_channels_are_independent(rsm, up, down):
    n = rs.edge_len(_T(rsm, up, down, 5), up, down) + 57
    x5 = np.ascontiguousarray(rs.white(8200 + up, n, 5))
    y5 = rsm.resample_poly(x5, up, down).cpu().numpy()
    y2 = rsm.resample_poly(np.ascontiguousarray(x5[:, 1:3]), up, down).cpu().numpy()
    for c in range(5):
        mono = rsm.resample_poly(np.ascontiguousarray(x5[:, c]), up, down).cpu().numpy()
        assert mono.shape == (y5.shape[0],)
        assert np.array_equal(_bits(mono), _bits(y5[:, c])), c
    assert np.array_equal(_bits(y2), _bits(y5[:, 1:3]))


def test_resample_to_and_copy(rsm):
    import torch
    x = np.ascontiguousarray(rs.white(8300, 4410 + 3, 5)[:, :2])
    y = rsm.resample_to(x, 44100, 48000, 100, 100 + 441)
    assert y.shape == (480, 2)
    want = rsm.resample_poly(x[100:541], 160, 147)
    assert torch.equal(y, want)
    # a ratio that reduces to 1 / 1 copies; 96 / 48 reduces to 2 / 1
    same = rsm.resample_poly(x, 3, 3, 5, 50)
    assert np.array_equal(same.cpu().numpy(), x[5:50])
    assert torch.equal(rsm.resample_poly(x, 96, 48), rsm.resample_poly(x, 2, 1))


# ---------------------------------------------------------------------------
# 4. guards
# ---------------------------------------------------------------------------

def test_entry_point_guards(rsm):
    import torch
    from tomatis_audio_processor_amd import _lib
    L = _lib.lib()
    x = torch.zeros(64 * 2, dtype=torch.float32, device="cuda")
    h = torch.zeros(20 * 512 + 3, dtype=torch.float32, device="cuda")
    out = torch.zeros(8 * 64 * 8, dtype=torch.float32, device="cuda")
    hs = _lib.stream_handle()
    p = _lib.ptr

    def call(xp=p(x), n_total=64, start=0, ln=64, ch=2, up=1, down=2, hp=p(h), n_taps=41,
             op=p(out)):
        return L.tomatis_resample_poly(xp, n_total, start, ln, ch, up, down, hp, n_taps, op, hs)

    assert call() == 0
    null = C.c_void_p(0)
    bad_arg = [dict(xp=null), dict(hp=null), dict(op=null), dict(start=-1), dict(ln=0),
               dict(start=1), dict(ln=65), dict(n_total=-1), dict(n_taps=40), dict(n_taps=0),
               dict(up=2, down=2), dict(up=1, down=1), dict(up=2, down=4), dict(up=6, down=4),
               dict(up=0), dict(down=0), dict(ch=0), dict(ch=9)]
    for kw in bad_arg:
        assert call(**kw) == _lib.E_ARG, kw
    unsupported = [dict(up=513, down=512, n_taps=41), dict(up=1, down=9), dict(up=3, down=25),
                   dict(up=512, down=513, n_taps=41), dict(n_taps=43),
                   dict(up=160, down=147, n_taps=3203)]
    for kw in unsupported:
        assert call(**kw) == _lib.E_UNSUPPORTED, kw
    for kw in [dict(up=512, down=511, n_taps=10241), dict(up=1, down=8, n_taps=161),
               dict(ch=8, n_total=16, ln=16)]:
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()


def test_value_errors(rsm):
    x = np.zeros((100, 2), np.float32)
    with pytest.raises(ValueError, match=r"max\(up, down\) <= 512 and down <= 8 up"):
        rsm.resample_poly(x, 1, 9)
    with pytest.raises(ValueError, match=r"max\(up, down\) <= 512"):
        rsm.resample_to(x, 44101, 48000)
    with pytest.raises(ValueError, match=r"1\.\.8 channels"):
        rsm.resample_poly(np.zeros((10, 9), np.float32), 1, 2)
    with pytest.raises(ValueError, match="non-empty range"):
        rsm.resample_poly(x, 1, 2, 50, 50)
    with pytest.raises(ValueError, match="non-empty range"):
        rsm.resample_poly(x, 1, 2, -1, 50)
    with pytest.raises(ValueError):
        rsm.resample_poly(np.zeros((2, 2, 2), np.float32), 1, 2)
