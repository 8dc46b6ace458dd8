"""GPU: the paths of the audio resampler (tm_resample.hip k_rs_poly) that
tests/test_gpu_resample.py never takes with checked values.

a. Revisited tiles.  The launch puts at most 4 x CUs workgroups on the device
   and each walks the tiles blockIdx.x, + gridDim.x, ...: an input of
   2 cap + cap / 2 + 1 tiles (T = 128 at 8 channels) makes every workgroup take
   two tiles and half of them a third, so the barrier in front of the staging,
   the reuse of the phase table and the tile stride run.  All outputs against
   float64; a sub-range that turns third-visit tiles into first-visit ones and
   a second run return the same bits.
b. K = 36 and K = 31 (4 / 7 and 2 / 3): K mod 4 of 0 (no padded zero tap) and 3,
   where every other tested ratio has 1 or 2.
c. Filters with no symmetry and of any odd length through the C entry point:
   seeded normal taps, n_taps from 1 (K = 1, phases without a tap) to the default.
d. An input that is not 16-byte aligned (a view into a resident buffer): the
   word-by-word staging does all the work and returns the aligned run's bits.
e. 3, 4, 6, 7 and 8 channels through the generic instantiation.

Values are judged as in test_gpu_resample.py: with y64 the float64 statement and
y32 a float32 evaluation of it, relative to the output peak,
    e = max |y - y64| / peak  <=  8 * max(e32, 2^-23),  e32 = the same of y32.
Every tile-edge length comes from ``resample.outputs_per_workgroup``, which
tests/test_resample_plan.py holds to the C plan.

Largest measured e / max(e32, 2^-23) on the MI355X: 0.98 (2 / 3 with 15 normal
taps, 23 frames), 0.87 (1 / 2 with 41 normal taps), 0.60 (2 / 3 and 4 / 7 with the
default filter), 0.55 and 0.32 over the 2561 revisited tiles (DESIGN.md §7i has
every case).
"""
import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import align_ref as ar
from tests import resample_ref as rs

pytestmark = pytest.mark.gpu


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


def _T(rsm, up, down, ch, n_taps=None):
    return rsm.outputs_per_workgroup(up, down, ch, n_taps)


def _report(tag, name, got, y64, y32):
    """The rule of 8; prints the RATIO line first."""
    assert got.dtype == np.float32 and got.shape == y64.shape == y32.shape
    peak = float(np.max(np.abs(y64)))
    assert peak > 0.0
    e32 = float(np.max(np.abs(y32.astype(np.float64) - y64)) / peak)
    e = float(np.max(np.abs(got.astype(np.float64) - y64)) / peak)
    print(f"RATIO [resample_poly {tag}] {name}: e {e:.3e} e32 {e32:.3e} "
          f"ratio {e / max(e32, ar.FLOOR):.2f}")
    assert e <= ar.bound(e32), (tag, name, e, e32)


# ---------------------------------------------------------------------------
# a. revisited tiles
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("up,down", [(512, 511), (1, 8)])
def test_revisited_tiles(rsm, up, down):
    import torch
    ch = 8
    cap = 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    T = _T(rsm, up, down, ch)
    assert T == 128                                   # the smallest tile of the domain
    want_tiles = 2 * cap + cap // 2 + 1
    n = ((want_tiles - 1) * T + T // 2 + 3) * down // up
    n_out = rsm.n_out(n, up, down)
    tiles = -(-n_out // T)
    assert tiles == want_tiles and tiles > 2 * cap and n_out % T != 0
    x = np.random.default_rng(9100 + up + down).uniform(-0.5, 0.5, (n, ch)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    full = rsm.resample_poly(xt, up, down).cpu().numpy()
    assert full.shape == (n_out, ch)
    K = -(-len(rsm.taps(up, down)) // up)
    _report(f"{up}/{down} K {K} ch {ch}", f"{tiles} tiles on {cap} workgroups", full,
            rs.resample_scipy64(x, up, down), resample_poly(x, up, down, axis=0))
    again = rsm.resample_poly(xt, up, down).cpu().numpy()
    assert np.array_equal(_bits(full), _bits(again)), "run to run"
    # the sub-range [down m, n): output j of it is output up m + j of the full run.  up m is
    # past cap tiles, so the tiles of a third visit become tiles of a first visit, and
    # where T does not divide up (1 / 8) at another offset inside the tile
    m = cap * T // up + 1 + (T // 2 if up % T else 0)
    assert up * m > cap * T and (up % T == 0 or (up * m) % T != 0)
    assert (2 * cap * T - up * m) // T < cap            # full's tile 2 cap: a first visit here
    sub = rsm.resample_poly(xt, up, down, down * m, n).cpu().numpy()
    assert sub.shape == (n_out - up * m, ch)
    j_lo = K * up // down + 2                          # from here the K frames lie inside both
    assert np.array_equal(_bits(full[up * m + j_lo:]), _bits(sub[j_lo:])), "independent of start"
    assert not np.array_equal(_bits(full[up * m:up * m + j_lo]), _bits(sub[:j_lo]))


# ---------------------------------------------------------------------------
# b. K mod 4 of 0 and 3
# ---------------------------------------------------------------------------

K_RATIOS = [(4, 7), (2, 3)]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("up,down", K_RATIOS)
def test_impulse_exact_k0_k3(rsm, up, down, ch):
    import torch
    h = rsm.taps(up, down)
    assert -(-len(h) // up) == {(4, 7): 36, (2, 3): 31}[(up, down)]
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
    start, i0 = 7, mid
    big = np.zeros((n + 20, ch), np.float32)
    big[start + i0, ch - 1] = 1.0
    y = rsm.resample_poly(torch.from_numpy(big).cuda(), up, down, start, start + n).cpu().numpy()
    want = rs.impulse_response(n, up, down, h, i0)
    assert np.array_equal(_bits(y[:, ch - 1]), _bits(want))


def _judge(rsm, x, up, down, name):
    h = rsm.taps(up, down)
    got = rsm.resample_poly(x, up, down).cpu().numpy()
    _report(f"{up}/{down} K {-(-len(h) // up)} ch {x.shape[1]}", name, got,
            rs.resample_direct(x, up, down, h, np.float64), resample_poly(x, up, down, axis=0))
    return got


@pytest.mark.parametrize("up,down,ch", [(4, 7, 2), (2, 3, 2), (4, 7, 1), (4, 7, 5)])
def test_against_float64_k0_k3(rsm, up, down, ch):
    n_t = rs.edge_len(_T(rsm, up, down, ch), up, down)
    lens = sorted({1, 2, 23, max(1, down - 1), down + 1, n_t, n_t + 1, 3 * n_t + 7, 8000 + 17})
    src = rs.white(7300 + up + down, max(lens), 5)
    for n in lens:
        _judge(rsm, np.ascontiguousarray(src[:n, :ch]), up, down, f"len {n}")


# ---------------------------------------------------------------------------
# c. asymmetric and short filters through the C entry point
# ---------------------------------------------------------------------------

CUSTOM = [(3, 2, 1), (3, 2, 5), (5, 3, 3), (7, 5, 13), (1, 2, 7), (2, 3, 15), (160, 147, 159),
          (160, 147, 161), (1, 2, 41), (160, 147, 3201)]


def _entry(x, up, down, h):
    """tomatis_resample_poly of the whole [n, ch] host array with the taps h."""
    import torch
    from tomatis_audio_processor_amd import _lib
    n, ch = x.shape
    xt = torch.from_numpy(np.array(x, np.float32)).cuda()    # a copy: the shared noise is read-only
    ht = torch.from_numpy(np.ascontiguousarray(h, np.float32)).cuda()
    out = torch.full((-(-n * up // down), ch), np.nan, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().tomatis_resample_poly(
        _lib.ptr(xt), n, 0, n, ch, up, down, _lib.ptr(ht), len(h), _lib.ptr(out),
        _lib.stream_handle()), "resample_poly")
    return out.cpu().numpy()


@pytest.mark.parametrize("up,down,n_taps", CUSTOM)
def test_custom_taps_impulse_exact(rsm, up, down, n_taps):
    ch = 2
    h = rs.random_taps(9300 + 7 * up + n_taps, n_taps)
    assert np.all(h != 0.0) and (n_taps < 3 or not np.array_equal(h, h[::-1]))
    T = _T(rsm, up, down, ch, n_taps)
    edge = rs.edge_len(T, up, down)
    n = edge + edge // 2 + 3
    where = [0, (T // 2 + 5) * down // up, n - 1, edge]
    if n_taps < up:   # an impulse may fall on no tap at all: take the neighbours too
        where += [1, where[1] + 1, n - 2, edge + 1]
    seen = 0
    for i0 in where:
        for c in (0, 1):
            y = _entry(rs.impulse(n, ch, i0, c), up, down, h)
            want = rs.impulse_response(n, up, down, h, i0)
            seen += int(np.count_nonzero(want))
            assert n_taps < up or np.any(want), (i0, c)
            assert np.array_equal(_bits(y[:, c]), _bits(want)), (i0, c)
            assert not np.any(_bits(y[:, 1 - c])), (i0, c)
    assert seen >= len(where) // 2


@pytest.mark.parametrize("up,down,n_taps", CUSTOM)
def test_custom_taps_against_float64(rsm, up, down, n_taps):
    ch = 2
    h = rs.random_taps(9300 + 7 * up + n_taps, n_taps)
    K = -(-n_taps // up)
    edge = rs.edge_len(_T(rsm, up, down, ch, n_taps), up, down)
    lens = [1, 23, edge, edge + 1, 2 * edge + 7]
    src = rs.white(9400 + up + n_taps, max(lens), 2)
    for n in lens:
        x = np.ascontiguousarray(src[:n])
        got = _entry(x, up, down, h)
        _report(f"{up}/{down} n_taps {n_taps} K {K} ch {ch}", f"len {n}", got,
                rs.resample_direct(x, up, down, h, np.float64),
                rs.resample_direct(x, up, down, h, np.float32))
        if n_taps < up:   # a phase without a tap: +0 whatever the samples are
            mask = rs.tapless(len(got), up, down, n_taps)
            assert mask.any() or n < max(lens)
            assert not np.any(_bits(got[mask])), n


# ---------------------------------------------------------------------------
# d. input not 16-byte aligned
# ---------------------------------------------------------------------------

def _view(torch, words, frames, ch):
    """A contiguous [frames, ch] ([frames] for mono) view `words` floats into a
    fresh resident buffer."""
    buf = torch.zeros(words + frames * ch + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[words:words + frames * ch]
    v = v if ch == 1 else v.view(frames, ch)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (words % 4) != 0
    return v


@pytest.mark.parametrize("ch,words", [(1, 1), (1, 2), (1, 3), (2, 2), (3, 3)])
@pytest.mark.parametrize("up,down", [(160, 147), (1, 2), (3, 2)])
def test_unaligned_input(rsm, up, down, ch, words):
    import torch
    n = 2 * rs.edge_len(_T(rsm, up, down, ch), up, down) + 11
    x = np.ascontiguousarray(rs.white(8500 + up, n, 5)[:, :ch])
    x = x[:, 0] if ch == 1 else x
    xt = torch.from_numpy(x.copy()).cuda()
    assert xt.data_ptr() % 16 == 0
    first = rsm.resample_poly(xt, up, down).cpu().numpy()
    v = _view(torch, words, n, ch)
    v.copy_(xt)
    got = rsm.resample_poly(v, up, down).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(got)), "the full range"
    # the range at an odd start inside a buffer of ones, ending before the buffer does
    start = 13
    v = _view(torch, words, n + 40, ch)
    v.fill_(1.0)
    v[start:start + n] = xt
    sub = rsm.resample_poly(v, up, down, start, start + n).cpu().numpy()
    assert np.array_equal(_bits(first), _bits(sub)), "a sub-range of a live buffer"


# ---------------------------------------------------------------------------
# e. 3, 4, 6, 7 and 8 channels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("up,down", [(160, 147), (1, 2), (1, 8)])
def test_generic_channel_counts(rsm, up, down):
    counts = (3, 4, 6, 7, 8)
    lens = {ch: rs.edge_len(_T(rsm, up, down, ch), up, down) + 57 for ch in counts}
    src = rs.white(8600 + up + down, max(lens.values()), 8)
    mono = {}
    for ch in counts:
        n = lens[ch]
        x = np.ascontiguousarray(src[:n, :ch])
        y = rsm.resample_poly(x, up, down).cpu().numpy()
        assert y.shape == (rsm.n_out(n, up, down), ch)
        for c in range(ch):
            if (c, n) not in mono:
                mono[c, n] = rsm.resample_poly(np.ascontiguousarray(x[:, c]), up, down).cpu().numpy()
            assert np.array_equal(_bits(mono[c, n]), _bits(y[:, c])), (ch, c)
        if ch == 8:
            h = rsm.taps(up, down)
            _report(f"{up}/{down} K {-(-len(h) // up)} ch 8", f"len {n}", y,
                    rs.resample_direct(x, up, down, h, np.float64),
                    resample_poly(x, up, down, axis=0))
