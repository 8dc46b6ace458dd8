"""GPU: per-bin fidelity of the transforms against float64 (tests/stft_ref.py).

Every other sample-level test of the STFT -> gain -> ISTFT -> overlap-add
kernels is a round trip through a smooth gain curve on a music-like signal,
judged at an absolute 1e-4.  Here the input is white, every bin of every gain
row is an independent random number in [0.25, 1], and the bound is tied to
float32 rounding: for one stream

    e = max |(y - y64) * sum w^2| / max |y64 * sum w^2|      (sum w^2 >= 1e-3)
    e <= FACTOR * max(e32, 2^-23),  FACTOR = 8

with y64 the float64 numpy statement of the operation and e32 the error of the
same statement run in float32, on the very same case.  tests/test_stft_ref.py
shows on the CPU that a gain landing on the neighbouring bin, a 5 % error in
one bin, or the mirrored half of the packed stereo spectrum reading g[k+1] each
exceed 32 * max(e32, 2^-23) on every (n_fft, hop) used here.

The pipelines' gain tables are overwritten on the device after construction
(they are read at run()); the input peak keeps the limiter off (asserted).
Gate states, alpha and r equal the oracle's bit for bit as elsewhere in the
suite, both gate states occur, and the per-frame row ids come from the
pipeline (``pipe.rows``; the fused gate keeps them in registers, there they
follow from the states it wrote).

The analysis spectra (tm_analysis.hip) are forward-only: mean |rfft| over
frames of white noise, largest per-bin relative error, same bound rule.

Largest measured e / max(e32, 2^-23) per path on the MI355X:

    2048 fast            1.27   (2048/512 mono cross-fade)
    4096                 1.31   (4096/2048 stereo cross-fade)
    generic hop          1.35   (2048/300 stereo)
    LDS pow2             1.52   (32/5, 5 channels)
    LDS Bluestein        2.14   (100/25 mono, pad)
    HBM                  1.72   (40000/10000 mono)
    analysis pow2        1.68   mono input (32/8); power-mono premix 4.06 up to
                                n_fft 4096, 8.85 at 8192, 14.10 at 16384
    analysis Bluestein   4.95   (8191, power-mono premix; mono input 2.09)

FACTOR 8 holds on every path but one: the analysis spectra of a power-mono
signal at the power-of-two lengths 8192 and 16384 run under the ceiling factor
32 (AN_PREMIX_POW2_FACTOR; measured 8.85 and 14.10).  A power-mono signal is
non-negative: its windowed mean puts 400 times a noise bin's magnitude into
bins 0 and +-1, and the radix-4 Stockham stages multiply those two neighbours
by rounded twiddles, whose error lands on the few bins k = +-1 mod N/4, N/16,
... (the worst bins are N/4, N/2 and their neighbours; the median bin sits at
6e-8).  The same factorisation run in float32 numpy on the 8192 input gives
9.0 where the device gives 8.85, and 1.4 on the mono input
(tests/test_stft_ref.py::test_premix_pow2_rounding_is_the_factorisation):
rounding of this factorisation, not a misplaced bin, which would be O(1).
"""
import functools

import numpy as np
import pytest

from oracle import tomatis_oracle as orc
from tests import stft_ref as sr
from tests.stft_ref import FACTOR, FLOOR, bound, case_rows, ola_error, stft_ref, white

pytestmark = pytest.mark.gpu
SR = 48000
DB_ATOL = 2e-3   # dB, as tests/test_gpu_analysis.py


def _engine():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import engine
    return torch, engine


def _dev_opts(**kw):
    from tomatis_audio_processor_amd._lib import dev_options
    return dev_options(**kw)


def _set_gains(torch, pipe, g):
    g = np.ascontiguousarray(g, np.float32)
    assert tuple(pipe.gains.shape) == g.shape
    pipe.gains.copy_(torch.from_numpy(g).to(pipe.gains.device))


def _reference(x, st, n_fft, hop, gains, rows, norm):
    """(y64, wsum64, e32) of plan stream ``st`` (its geometry as the C ABI got it)."""
    win = np.hanning(n_fft).astype(np.float32)
    kw = dict(first_start=int(st.first_start), n_frames=int(st.n_frames), hop=hop,
              out_begin=int(st.out_begin), out_len=int(st.out_len),
              in_scale=float(st.in_scale), norm=norm)
    y64, w64, _ = stft_ref(x, win, gains, rows, **kw)
    y32, _, _ = stft_ref(x, win, gains, rows, dtype=np.float32, **kw)
    return y64, w64, ola_error(y32, y64, w64)


def _judge(path, name, y, ref, factor=FACTOR):
    y64, w64, e32 = ref
    assert y.shape == y64.shape
    e = ola_error(y, y64, w64)
    print(f"RATIO [{path}] {name}: e {e:.3e} e32 {e32:.3e} ratio {e / max(e32, FLOOR):.2f}")
    assert e <= bound(e32, factor), (path, name, e, e32)
    return e


# ---------------------------------------------------------------------------
# register kernels (n_fft 2048 / 4096) and the generic hop: gate pipelines
# ---------------------------------------------------------------------------

def _gate_len(n_fft, hop, m):
    """m + n_fft / hop + 2 frames of the standard schedule (half a hop of end
    pad)."""
    return n_fft + m * hop + hop // 2


def _gate_params(n_fft, hop, amp):
    """Loud blocks at amp / sqrt(3) RMS, quiet ones 30 dB below, the threshold
    half way; an up-delay of 4.5 frames (row 0 meets loud frames too)."""
    T = 20.0 * np.log10(amp / np.sqrt(3.0)) - 15.0
    return dict(gate_ui=T + 100.0, gate_mode="linear", n_fft=n_fft, hop=hop,
                up_delay_ms=4.5 * hop / SR * 1000.0)


def _xfade_rows(states, alpha, xf):
    a = np.asarray(alpha, np.float64)
    mid = (a > 0.0) & (a < 1.0) if xf > 0 else np.zeros(len(a), bool)
    return np.where(mid, 2 + np.rint(a * xf).astype(np.int64), (a >= 0.5).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _gate_case(seed, n_fft, hop, ch, m, xfade, sep=None):
    """(x, params, oracle result, row ids by the reference rule)."""
    amp = 0.5
    wk = dict(silent=(1,)) if sep == "silent" else dict(scaled=(1,)) if sep == "scaled" else {}
    x = white(seed, _gate_len(n_fft, hop, m), ch, amp=amp, block=16 * hop, **wk)
    # the last samples lie under the tail of the last frame alone, where
    # 1 / sum w^2 would blow them up into the limiter: that frame is silent
    x[-n_fft:] = 0.0
    p = _gate_params(n_fft, hop, amp)
    if xfade:
        p["xfade_ms"] = 5.5 * hop / SR * 1000.0
    ref = orc.process_standard(x, SR, **p)
    assert set(np.unique(ref["states"])) == {1, 2}, "both gate states must occur"
    if xfade:
        rows = _xfade_rows(ref["states"], ref["alpha"], 6)
        assert len(set(rows[rows > 1])) >= 3, "lattice rows must occur"
    else:
        rows = ref["states"].astype(np.int64) - 1
    x.setflags(write=False)
    return x, p, ref, rows


def _check_gate(torch, E, path, name, pipe, res, x, oref, rows_ref, g, i=0, two_pass_rows=True):
    """Stream ``i`` of a GatePipeline run against the oracle's gate and the
    float64 statement of the transform."""
    st = pipe.plan.streams[i]
    F = int(st.n_frames)
    assert np.array_equal(res.stream_states(i), oref["states"])
    assert np.array_equal(res.stream_r(i).view(np.uint32),
                          np.asarray(oref["r"], np.float32).view(np.uint32))
    if oref["alpha"] is not None:
        assert np.array_equal(res.stream_alpha(i), oref["alpha"])
    if two_pass_rows:
        a = int(st.frame_base)
        rows = pipe.rows[a:a + F].cpu().numpy().astype(np.int64)
        assert np.array_equal(rows, rows_ref)
    else:
        rows = rows_ref
    ref = _reference(x, st, pipe.n_fft, pipe.hop, g, rows, "eps")
    assert float(np.abs(ref[0]).max()) < 0.9, "reference peak: the limiter must stay off"
    assert float(res.stream_peaks(i).max()) <= 0.999
    return _judge(path, name, res.output(i), ref), ref


def _run_gate(torch, E, path, seed, n_fft, hop, ch, m, *, xfade=False, fused=True,
              expect_gated=None, sep=None):
    x, p, oref, rows_ref = _gate_case(seed, n_fft, hop, ch, m, xfade, sep)
    ss = E.StreamSet.from_arrays([x], SR)
    pipe = E.GatePipeline(ss, fused_levels=fused, **p)
    g = case_rows(seed + 50, pipe.n_rows, n_fft // 2 + 1)
    _set_gains(torch, pipe, g)
    res = pipe.run()
    if expect_gated is not None:
        assert pipe.gated_used == expect_gated
    name = f"{n_fft}/{hop} ch{ch} {'xfade' if xfade else 'std'} " \
           f"{'gated' if pipe.gated_used else 'two-pass'}{' ' + sep if sep else ''}"
    _check_gate(torch, E, path, name, pipe, res, x, oref, rows_ref, g,
                two_pass_rows=not pipe.gated_used)
    return pipe, g, x, oref, rows_ref


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("hop", [256, 512, 1024])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twopass"])
def test_fast_2048_gate(hop, ch, fused):
    """n_fft 2048 register kernel (single-exchange FFT, gains in LDS), ~130
    frames (interior run and edge runs): fused gate (hop 256 / 512; hop 1024
    declines it) and the two-pass chain."""
    torch, E = _engine()
    _run_gate(torch, E, "2048 fast", 100 + hop + ch, 2048, hop, ch, 124, fused=fused,
              expect_gated=fused and hop != 1024)


@pytest.mark.parametrize("hop,ch", [(512, 2), (512, 1), (256, 2)])
def test_fast_2048_xfade(hop, ch):
    """Cross-fade at 2048: every lattice row random (mixed rows in LDS)."""
    torch, E = _engine()
    pipe, *_ = _run_gate(torch, E, "2048 fast", 200 + hop + ch, 2048, hop, ch, 124, xfade=True)
    assert pipe.n_rows == 9


def _adaptive_case(seed, n_fft, hop, ch, m):
    # peak <= -17 dBFS: no attenuation (in_scale = out_scale = 1); a silent
    # first frame: the only frame over [0, hop) adds exact zeros there, where
    # max(sum w^2, 1e-8) would otherwise blow the first samples up
    x = white(seed, _gate_len(n_fft, hop, m), ch, amp=0.125, block=16 * hop)
    x[:n_fft] = 0.0
    p = dict(n_fft=n_fft, hop=hop, min_hold_ms=3.5 * hop / SR * 1000.0,
             xfade_ms=5.5 * hop / SR * 1000.0)
    return x, p, orc.process_adaptive(x, SR, **p)


@pytest.mark.parametrize("n_fft,hop,ch,path", [(2048, 512, 2, "2048 fast"), (2048, 256, 1, "2048 fast"),
                                               (4096, 1024, 2, "4096")])
def test_adaptive_max_norm(n_fft, hop, ch, path):
    """AdaptivePipeline: max(sum w^2, 1e-8) normalisation, rows 2 + m."""
    torch, E = _engine()
    x, p, oref = _adaptive_case(300 + hop + ch, n_fft, hop, ch, 124 if n_fft == 2048 else 64)
    assert oref["atten_db"] == 0 and oref["scale"] is None
    assert set(np.unique(oref["states"])) == {1, 2}
    ss = E.StreamSet.from_arrays([x], SR)
    pipe = E.AdaptivePipeline(ss, **p)
    g = case_rows(350 + hop, pipe.n_rows, n_fft // 2 + 1)
    _set_gains(torch, pipe, g)
    res = pipe.run()
    assert res.extra["atten_db"][0] == 0
    assert np.array_equal(res.stream_states(0), oref["states"])
    assert np.array_equal(res.stream_alpha(0), oref["alpha"])
    assert float(res.extra["thresholds"].cpu().numpy()[0]) == oref["threshold"]
    st = pipe.plan.streams[0]
    F = int(st.n_frames)
    rows = pipe.rows[int(st.frame_base):int(st.frame_base) + F].cpu().numpy().astype(np.int64)
    assert np.array_equal(rows, 2 + np.rint(oref["alpha"] * pipe.xf).astype(np.int64))
    assert len(set(rows)) >= 4
    ref = _reference(x, st, n_fft, hop, g, rows, "max")
    assert float(np.abs(ref[0]).max()) < 0.9 and float(res.stream_peaks(0).max()) <= 0.999
    _judge(path, f"{n_fft}/{hop} ch{ch} adaptive", res.output(0), ref)


def test_fast_2048_pipelined_pair():
    """Two pipelined passes on two different inputs: each pass's output is
    limited inside the next launch (or the flush); both are checked."""
    torch, E = _engine()
    n_fft, hop, ch = 2048, 512, 2
    xa, p, ora, rows_a = _gate_case(401, n_fft, hop, ch, 124, False)
    xb, _, orb, rows_b = _gate_case(402, n_fft, hop, ch, 124, False)
    ss = E.StreamSet.from_arrays([xa], SR)
    pipe = E.GatePipeline(ss, pipelined=True, **p)
    g = case_rows(403, pipe.n_rows, n_fft // 2 + 1)
    _set_gains(torch, pipe, g)
    assert pipe.run() is None and pipe.pending and pipe.pipelined and pipe.gated_used
    ya_dev, st_a, r_a = pipe.y, pipe.states.clone(), pipe.r.clone()
    ss.x.copy_(torch.from_numpy(np.array(xb).reshape(-1)).to(ss.x.device))
    assert pipe.run() is None and pipe.pending
    res = pipe.result()
    st = pipe.plan.streams[0]
    F, N = int(st.n_frames), len(xa)
    # second pass: the result as returned
    _check_gate(torch, E, "2048 fast", "2048/512 ch2 pipelined pass 2", pipe, res, xb, orb,
                rows_b, g, two_pass_rows=False)
    # first pass: its buffer, final since the second launch
    assert np.array_equal(st_a[:F].cpu().numpy(), ora["states"])
    assert np.array_equal(r_a[:F].cpu().numpy().view(np.uint32),
                          np.asarray(ora["r"], np.float32).view(np.uint32))
    ref = _reference(xa, st, n_fft, hop, g, rows_a, "eps")
    assert float(np.abs(ref[0]).max()) < 0.9
    ya = ya_dev[res.out_offs[0]:res.out_offs[0] + N * ch].cpu().numpy().reshape(N, ch)
    _judge("2048 fast", "2048/512 ch2 pipelined pass 1", ya, ref)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("hop", [512, 1024, 2048])
@pytest.mark.parametrize("xfade", [False, True], ids=["std", "xfade"])
def test_reg_4096(hop, ch, xfade):
    """n_fft 4096 register kernel (two waves per frame, gains in L2), ~70 frames."""
    torch, E = _engine()
    _run_gate(torch, E, "4096", 500 + hop + ch, 4096, hop, ch, 64, xfade=xfade,
              expect_gated=False)


def test_reg_4096_fused():
    torch, E = _engine()
    with _dev_opts(FUSED_4096=1):
        _run_gate(torch, E, "4096", 601, 4096, 1024, 2, 64, expect_gated=True)


@pytest.mark.parametrize("n_fft,hop,ch", [(2048, 300, 2), (4096, 1000, 1), (2048, 300, 1),
                                          (4096, 1000, 2)])
def test_generic_hop(n_fft, hop, ch):
    """k_stft_frames (fft_fwd / fft_inv) behind hops the register emit blocks
    do not take."""
    torch, E = _engine()
    _run_gate(torch, E, "generic hop", 700 + hop + ch, n_fft, hop, ch, 40, expect_gated=False)


def test_generic_hop_p64_off():
    """n_fft 2048 in the 128 x 16 register layout."""
    torch, E = _engine()
    with _dev_opts(P64=0):
        _run_gate(torch, E, "generic hop", 750, 2048, 512, 2, 124, fused=False)


# ---------------------------------------------------------------------------
# static EQ: hop == n_fft on the register sizes, the any-size path
# ---------------------------------------------------------------------------

def _static_len(n_fft, hop, pad, frames):
    if pad:   # F = N // hop + 1
        return (frames - 1) * hop + min(3, hop - 1)
    return n_fft + (frames - 1) * hop + min(3, hop - 1)


def _run_static(torch, E, path, xs, n_fft, hop, pad, g, name, factor=FACTOR):
    ss = E.StreamSet.from_arrays(xs, SR)
    pipe = E.StaticEqPipeline(ss, g[0], n_fft=n_fft, hop=hop, pad=pad)
    res = pipe.run()
    refs = []
    for i, x in enumerate(xs):
        st = pipe.plan.streams[i]
        y = res.output(i)
        if st.out_len == 0:
            assert y.size == 0
            refs.append(None)
            continue
        ref = _reference(x, st, n_fft, hop, g, np.zeros(int(st.n_frames), np.int64), "eps")
        _judge(path, f"{name} stream {i}", y, ref, factor)
        refs.append(ref)
    return pipe, res, refs


def _static_both(torch, E, path, n_fft, hop, ch, frames=6, full_frame=True, **wk):
    g = case_rows(8000 + n_fft, 1, n_fft // 2 + 1)
    for pad in (False, True):
        N = _static_len(n_fft, hop, pad, frames)
        if pad and N < n_fft and full_frame:   # at least one frame's worth of samples
            N += n_fft
        x = white(n_fft * 3 + hop + pad, N, ch, **wk)
        _run_static(torch, E, path, [x], n_fft, hop, pad, g,
                    f"{n_fft}/{hop} ch{ch} {'pad' if pad else 'nopad'}")


def test_generic_hop_2048_2048():
    """hop == n_fft (no overlap: sum w^2 reaches zero at every frame edge, so
    the static pass, which has no limiter, carries this shape)."""
    torch, E = _engine()
    _static_both(torch, E, "generic hop", 2048, 2048, 2, frames=8)


_CH = (1, 2, 3, 5)


@pytest.mark.parametrize("n_fft,hop,ch", [(n, h, _CH[i % 4]) for i, (n, h) in enumerate(sr.LDS_POW2)]
                         + [(n, h, 3) for n, h in sr.LDS_POW2_3CH])
def test_lds_pow2(n_fft, hop, ch):
    """Any-size path in LDS, Stockham powers of two (2048 / 4096: three
    channels force the path)."""
    torch, E = _engine()
    _static_both(torch, E, "LDS pow2", n_fft, hop, ch)


def test_lds_n_fft_2_is_zero():
    """np.hanning(2) is all zero: exact zeros out."""
    torch, E = _engine()
    x = white(2, 40, 2)
    ss = E.StreamSet.from_arrays([x], SR)
    for pad in (False, True):
        res = E.StaticEqPipeline(ss, case_rows(2, 1, 2)[0], n_fft=2, hop=1, pad=pad).run()
        y = res.output(0)
        assert y.shape[0] >= 39 and not y.any()


@pytest.mark.parametrize("n_fft,hop,ch", [(n, h, _CH[(i + 1) % 4])
                                          for i, (n, h) in enumerate(sr.LDS_BLUESTEIN)])
def test_lds_bluestein(n_fft, hop, ch):
    """Any-size path in LDS, Bluestein lengths on every M and at its edges."""
    torch, E = _engine()
    _static_both(torch, E, "LDS Bluestein", n_fft, hop, ch)


@pytest.mark.parametrize("n_fft,hop,ch", [(32768, 8192, 2), (65536, 16384, 1), (8193, 2048, 2),
                                          (40000, 10000, 1)])
def test_hbm(n_fft, hop, ch):
    """Any-size path with per-block HBM buffers (FFT above the LDS)."""
    torch, E = _engine()
    _static_both(torch, E, "HBM", n_fft, hop, ch, frames=4, full_frame=False)


# ---------------------------------------------------------------------------
# channel separation, ragged batches, end-to-end sensitivity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("sep", ["silent", "scaled"])
@pytest.mark.parametrize("path,n_fft,hop", [("2048 fast", 2048, 512), ("4096", 4096, 1024),
                                            ("generic hop", 2048, 300)])
def test_channel_separation_gate(path, n_fft, hop, sep):
    """Stereo with the right channel silent, then at 1e-3 of the left: L + iR
    packing is exact only while the permuted table is symmetric.  Same measure
    (the silent channel's reference is exactly zero)."""
    torch, E = _engine()
    m = {2048: 124, 4096: 64}[n_fft] if hop != 300 else 40
    _, g, x, oref, rows = _run_gate(torch, E, path, 900 + hop, n_fft, hop, 2, m, sep=sep)
    if sep == "silent":
        assert not x[:, 1].any()


@pytest.mark.parametrize("sep", ["silent", "scaled"])
@pytest.mark.parametrize("path,n_fft,hop", [("LDS pow2", 256, 100), ("LDS Bluestein", 100, 25),
                                            ("HBM", 8193, 2048)])
def test_channel_separation_static(path, n_fft, hop, sep):
    torch, E = _engine()
    wk = dict(silent=(1,)) if sep == "silent" else dict(scaled=(1,))
    g = case_rows(8000 + n_fft, 1, n_fft // 2 + 1)
    x = white(950 + n_fft, _static_len(n_fft, hop, True, 6) + n_fft, 2, **wk)
    _, _, refs = _run_static(torch, E, path, [x], n_fft, hop, True, g, f"{n_fft}/{hop} ch2 {sep}")
    if sep == "silent":
        assert not refs[0][0][:, 1].any()


def test_ragged_anysize():
    """Three streams in one any-size plan, one shorter than a frame (no pad: no
    frame, no output; pad: partial frames only)."""
    torch, E = _engine()
    n_fft, hop = 100, 25
    g = case_rows(8000 + n_fft, 1, n_fft // 2 + 1)
    xs = [white(960 + i, n, 2) for i, n in enumerate([1000, 60, 517])]
    pipe, res, refs = _run_static(torch, E, "LDS Bluestein", xs, n_fft, hop, False, g, "ragged 100/25 nopad")
    assert refs[1] is None and res.out_lens[1] == 0
    _, _, refs = _run_static(torch, E, "LDS Bluestein", xs, n_fft, hop, True, g, "ragged 100/25 pad")
    assert all(r is not None for r in refs)


def test_ragged_2048():
    """Three streams in one n_fft 2048 plan (interior run, short streams in
    generic edge runs), one shorter than a frame."""
    torch, E = _engine()
    n_fft, hop = 2048, 512
    g = case_rows(8000 + n_fft, 1, n_fft // 2 + 1)
    xs = [white(970 + i, n, 2) for i, n in enumerate([130 * hop + 77, 1500, 9 * hop + 301])]
    _, _, refs = _run_static(torch, E, "2048 fast", xs, n_fft, hop, True, g, "ragged 2048/512 pad")
    assert all(r is not None for r in refs)


def _assert_sensitive(path, name, y, ref):
    """A run with two neighbouring gains swapped on the device is farther from
    the unmutated reference than the bound: the kernel reads those bins."""
    e = ola_error(y, ref[0], ref[1])
    print(f"SWAP [{path}] {name}: e {e:.3e} bound {bound(ref[2]):.3e}")
    assert e > bound(ref[2]), (path, name, e, ref[2])


@pytest.mark.parametrize("path,n_fft,hop,m", [("2048 fast", 2048, 512, 124), ("4096", 4096, 1024, 64),
                                              ("generic hop", 2048, 300, 40)])
def test_sensitivity_gate(path, n_fft, hop, m):
    torch, E = _engine()
    seed = 900 + hop   # the channel-separation case's twin, both channels live
    x, p, oref, rows_ref = _gate_case(seed, n_fft, hop, 2, m, False)
    ss = E.StreamSet.from_arrays([x], SR)
    pipe = E.GatePipeline(ss, **p)
    g = case_rows(seed + 50, pipe.n_rows, n_fft // 2 + 1)
    _set_gains(torch, pipe, g)
    res = pipe.run()
    _, ref = _check_gate(torch, E, path, f"{n_fft}/{hop} ch2 (sensitivity base)", pipe, res, x,
                         oref, rows_ref, g, two_pass_rows=not pipe.gated_used)
    gs, k = sr.swapped(g, row=1)   # the loud frames' row
    _set_gains(torch, pipe, gs)
    res = pipe.run()
    _assert_sensitive(path, f"{n_fft}/{hop} row 1 bins {k},{k + 1}", res.output(0), ref)


@pytest.mark.parametrize("path,n_fft,hop", [("LDS Bluestein", 1999, 500), ("HBM", 8193, 2048)])
def test_sensitivity_static(path, n_fft, hop):
    torch, E = _engine()
    g = case_rows(8000 + n_fft, 1, n_fft // 2 + 1)
    x = white(980 + n_fft, _static_len(n_fft, hop, True, 6) + n_fft, 2)
    pipe, res, refs = _run_static(torch, E, path, [x], n_fft, hop, True, g,
                                  f"{n_fft}/{hop} ch2 (sensitivity base)")
    gs, k = sr.swapped(g)
    _set_gains(torch, pipe, gs)
    res = pipe.run()
    _assert_sensitive(path, f"{n_fft}/{hop} bins {k},{k + 1}", res.output(0), refs[0])


# ---------------------------------------------------------------------------
# analysis spectra (tm_analysis.hip)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def an():
    torch, _ = _engine()
    from tomatis_audio_processor_amd import analysis, _lib
    _lib.lib()
    return analysis


def _mag_avg(sig, n_fft, hop, dt):
    """mean over frames of |rfft(frame * w)|, one frame at a time, in ``dt``."""
    w = np.hanning(n_fft).astype(np.float32).astype(dt)
    F = 1 + (len(sig) - n_fft) // hop
    acc = np.zeros(n_fft // 2 + 1, dt)
    for f in range(F):
        acc += np.abs(np.fft.rfft(sig[f * hop:f * hop + n_fft].astype(dt) * w)).astype(dt)
    return acc / dt(F)


# power-mono premix at n_fft 8192 / 16384 (Stockham, no Bluestein): measured
# ratios 8.85 / 14.10, the rounded twiddles on the DC neighbours of a
# non-negative signal (module docstring); the ceiling, not a fitted value
AN_PREMIX_POW2_FACTOR = sr.FACTOR_CEIL
AN_POW2 = [1 << k for k in range(4, 15)]
AN_BLUESTEIN = [17, 31, 33, 127, 129, 257, 513, 1025, 2049, 4097, 8191]


@pytest.mark.parametrize("n_fft", AN_POW2 + AN_BLUESTEIN)
def test_analysis_mag_avg(an, n_fft):
    """stft_mag_avg on white noise, 10 frames, mono and stereo through the
    power-mono premix: largest per-bin relative error against float64."""
    pow2 = n_fft & (n_fft - 1) == 0
    path = "analysis pow2" if pow2 else "analysis Bluestein"
    hop = max(1, n_fft // 4)
    x = white(1100 + n_fft, n_fft + 9 * hop + 1, 2)
    for premix in (None, "power_mono"):
        if premix:
            x64 = x.astype(np.float64)
            sig64 = np.sqrt(0.5 * (x64[:, 0] ** 2 + x64[:, 1] ** 2) + 1e-12)
            sig32 = np.sqrt(np.float32(0.5) * (x[:, 0] ** 2 + x[:, 1] ** 2) + np.float32(1e-12))
            got = an.stft_mag_avg(x, SR, n_fft, hop, premix="power_mono")
        else:
            sig64, sig32 = x[:, 0].astype(np.float64), x[:, 0]
            got = an.stft_mag_avg(x[:, 0].copy(), SR, n_fft, hop)
        m64 = _mag_avg(sig64, n_fft, hop, np.float64)
        m32 = _mag_avg(sig32, n_fft, hop, np.float32)
        assert m32.dtype == np.float32 and got.shape == m64.shape
        assert float(m64.min()) > 1e-4 * float(m64.max()), "every bin away from zero"
        e32 = float(np.max(np.abs(m32 - m64) / m64))
        e = float(np.max(np.abs(got - m64) / m64))
        print(f"RATIO [{path}] {n_fft}/{hop} {premix or 'mono'}: e {e:.3e} e32 {e32:.3e} "
              f"ratio {e / max(e32, FLOOR):.2f}")
        factor = AN_PREMIX_POW2_FACTOR if (premix and pow2 and n_fft >= 8192) else FACTOR
        assert e <= bound(e32, factor), (n_fft, premix, e, e32)


def test_analysis_logpower_median_small(an):
    """stft_logpower_median at n_fft 64 (an M no golden reaches) against the
    oracle's function on the same noise."""
    x = white(1201, 64 + 16 * 119, 2)
    f, med, used = an.stft_logpower_median(x, SR, 64, 16, -65.0)
    fr, mr, ur = orc.stft_logpower_median(x, SR, 64, 16, -65.0)
    assert used == ur == 120 and np.array_equal(f, fr)
    assert float(np.max(np.abs(med - mr))) <= DB_ATOL


def test_analysis_conditional_spectrum_small(an):
    """compute_conditional_spectrum at n_fft 129 (Bluestein, M = 512)."""
    n_fft, hop, F = 129, 32, 120
    x = white(1202, n_fft + hop * (F - 1), 2)
    y = (0.5 * x + 0.25 * white(1203, len(x), 2)).astype(np.float32)
    states = ["C1" if (k // 12) % 2 == 0 else "C2" for k in range(F)]
    f, c1, c2, n1, n2 = an.compute_conditional_spectrum(x, y, SR, states, n_fft, hop, -60)
    fr, r1, r2, m1, m2 = orc.compute_conditional_spectrum(x, y, SR, states, n_fft, hop, -60)
    assert (n1, n2) == (m1, m2) and n1 > 20 and n2 > 20 and np.array_equal(f, fr)
    assert float(np.max(np.abs(c1 - r1))) <= DB_ATOL
    assert float(np.max(np.abs(c2 - r2))) <= DB_ATOL
