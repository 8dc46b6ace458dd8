"""GPU: every output sample of the device, the ill-conditioned heads and tails
included, against the error model of conditioning.py (tests/edge_ref.py).

Every other sample-level test masks the samples with sum w^2 < TAU = 1e-3;
``Result.scale_flags()`` trusts the device's own values there.  Here, for
streams of 5 to 9 frames in every tail class of the framing,

    |y_dev(p) - y64(p)| <= D(p) = KAPPA_INT * A(p) + KAPPA_EDGE * A(p) * S1(p) / den(S2(p))

for EVERY output sample of every channel, y64 the float64 statement
(tests/stft_ref.py), and y_dev(p) == 0.0 exactly where D(p) == 0.  The
constants are conditioning.py's.  tests/test_edge_ref.py shows on the CPU that
numpy's float32 run meets D / 4 on the very same cases and that an
overlap-add that drops the last frame's tail, or a normaliser that reads the
window sum one sample late, exceeds D on masked samples.

Limiter: standard mode runs with an output gain of 2^-24 (exact in float32),
which keeps 1 / sum w^2 times the filter's tail under the limit (asserted);
the static pass has no limiter.  Cross-fade and adaptive plans have no output
gain: there the device's scale float32(0.999) / float32(peak) is divided out of
the chunk and 2^-23 |y| added to the bound.

Largest measured err / D per path on the MI355X, all samples / the masked
ones (sum w^2 < TAU), and numpy float32 on the same cases
(profiles/edge_samples/gpu_tests_edge_samples.log):

                                      device          numpy float32
    gated 2048 (2048/512, /256)       0.172 / 0.172   0.159 / 0.159
    4096 (4096/1024)                  0.164 / 0.158   0.128 / 0.128
    generic hop (2048/300)            0.152 / 0.152   0.156 / 0.156
    4096 cross-fade (4096/2048)       0.150 / 0.150   0.114 / 0.113
    adaptive 2048/512                 0.146 / 0.146   0.133 / 0.133
    adaptive LDS pow2 (1024/256)      0.130 / 0.130   0.098 / 0.092
    adaptive LDS Bluestein (3000/750) 0.168 / 0.140   0.111 / 0.078
    static 4096/2048                  0.189 / 0.189   0.156 / 0.156
    static LDS pow2 (512/128, 3 ch)   0.168 / 0.168   0.147 / 0.147
    static LDS Bluestein (100/25)     0.289 / 0.270   0.205 / 0.205
    static HBM (12000/3000 mono)      0.232 / 0.232   0.157 / 0.157

The device obeys the model on every path with a margin of 3.4 or more: no
kernel change, no recalibration, every extended shape kept.  What the cases
did find is host-side: at 2048/300 a stream with pe == 0 ends 124 samples
after its last frame, and the engine asked the plan for output there, which
tomatis_plan_create refuses (``test_last_frame_short_of_n``).
"""
import numpy as np
import pytest

from tests import edge_ref as er
from tomatis_audio_processor_amd import conditioning as cd

pytestmark = pytest.mark.gpu
SR = er.SR
LIMIT = np.float32(0.999)


def _engine():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import engine
    return torch, engine


def _set_gains(torch, pipe, g):
    g = np.array(g, np.float32, order="C")   # (a writable copy: the cases are read-only)
    assert tuple(pipe.gains.shape) == g.shape
    pipe.gains.copy_(torch.from_numpy(g).to(pipe.gains.device))


def _run(torch, E, cs, fused=True, own_gains=False):
    """One launch over the built cases ``cs`` (same mode, shape, channels and
    gain table) -> (pipe, res).  Geometry, gate states, alpha and row ids are
    the reference's (asserted).  ``own_gains``: keep the pipeline's tilt rows."""
    c0 = cs[0]
    assert all((c.mode, c.n_fft, c.hop, c.ch) == (c0.mode, c0.n_fft, c0.hop, c0.ch) for c in cs)
    ss = E.StreamSet.from_arrays([c.x for c in cs], SR)
    off = 0
    for c, o in zip(cs, ss.offs):   # packed: a tail directly before the next head
        assert o == off
        off += c.x.size
    if c0.mode in ("std", "xfade"):
        pipe = E.GatePipeline(ss, fused_levels=fused, **c0.params)
        assert pipe.n_rows == c0.n_rows
        if not own_gains:
            _set_gains(torch, pipe, c0.gains)
    elif c0.mode == "adaptive":
        pipe = E.AdaptivePipeline(ss, **c0.params)
        assert pipe.n_rows == c0.n_rows and pipe.xf == c0.xf
        _set_gains(torch, pipe, c0.gains)
    else:
        pipe = E.StaticEqPipeline(ss, c0.gains[0], n_fft=c0.n_fft, hop=c0.hop,
                                  pad=c0.mode == "static_pad")
    res = pipe.run()
    for i, c in enumerate(cs):
        st = pipe.plan.streams[i]
        # (the plan's out_len stops at the last frame's end; the result has the
        # reference's length, zeros beyond)
        geom = dict(first_start=int(st.first_start), n_frames=int(st.n_frames), hop=pipe.hop,
                    out_begin=int(st.out_begin), out_len=int(res.out_lens[i]))
        assert geom == c.geom, (geom, c.geom)
        end = geom["first_start"] + (geom["n_frames"] - 1) * pipe.hop + pipe.n_fft - geom["out_begin"]
        assert int(st.out_len) == min(geom["out_len"], end)
        assert float(st.in_scale) == 1.0 and float(st.out_scale) == c.out_scale
        if c.oref is None:
            continue
        a, F = int(st.frame_base), int(st.n_frames)
        assert np.array_equal(res.stream_states(i), c.oref["states"])
        if c.mode != "std":
            assert np.array_equal(res.stream_alpha(i), c.oref["alpha"])
        if c.mode == "adaptive":
            assert res.extra["atten_db"][i] == 0
            assert float(res.extra["thresholds"].cpu().numpy()[i]) == c.oref["threshold"]
        if not getattr(pipe, "gated_used", False):   # (the fused gate keeps its rows in registers)
            rows = pipe.rows[a:a + F].cpu().numpy().astype(np.int64)
            assert np.array_equal(rows, c.rows)
    return pipe, res


def _unlimited(res, i):
    """(stream i before the limiter as float64, the rounding its scale added
    per sample, chunks limited): the device's float32 scale divided out of
    every limited chunk."""
    y = res.output(i).astype(np.float64)
    extra = np.zeros(len(y))
    limited = 0
    if res.extra.get("limiter_applied", False):
        peaks = res.stream_peaks(i)
        for (a, b), pk in zip(res.chunk_ranges(i), peaks):
            if np.float32(pk) > LIMIT:
                y[a:b] /= np.float64(LIMIT / np.float32(pk))
                extra[a:b] = 2.0 ** -23 * np.abs(y[a:b]).max(axis=1)
                limited += 1
    return y, extra, limited


def _assert_bound(name, c, ref, y, extra=None):
    """The per-sample assertion on one stream; prints the measured ratios."""
    _, y64, s1, s2, D = ref
    assert y.shape == y64.shape
    err = np.abs(y - y64).max(axis=1)
    r_all, r_masked, _ = er.ratios(y, y64, D, s2)
    y32, _, _ = er.run_ref(c, dtype=np.float32)
    n_all, n_masked, _ = er.ratios(y32, y64, D, s2)
    print(f"RATIO [edge {c.path}] {name}: device max err/D all {r_all:.3f} / masked {r_masked:.3f}; "
          f"numpy float32 {n_all:.3f} / {n_masked:.3f}")
    bound = D if extra is None else D + extra
    bad = np.nonzero(err > bound)[0]
    assert len(bad) == 0, (name, "samples over D", bad[:8], err[bad[:8]], D[bad[:8]], s2[bad[:8]])
    zero = D == 0
    assert not y[zero].any(), (name, "nonzero output where D == 0", np.nonzero(zero)[0][:8])
    return r_all, r_masked


def _assert_peaks_are_the_samples(res, i, y):
    """Every chunk's peak is max |y| over the chunk, bit for bit (``y``: the
    device's float32 output, no limiter applied)."""
    peaks = res.stream_peaks(i)
    ranges = res.chunk_ranges(i)
    assert len(peaks) == len(ranges)
    for (a, b), pk in zip(ranges, peaks):
        want = np.abs(y[a:b]).max() if b > a else np.float32(0)
        assert np.float32(pk).view(np.uint32) == np.float32(want).view(np.uint32), (a, b, pk, want)


# ---------------------------------------------------------------------------
# a. per-sample bound on every path, every tail class
# ---------------------------------------------------------------------------

def _single(case, fused=True):
    torch, E = _engine()
    ref = er.reference(case)
    c = ref[0]
    pipe, res = _run(torch, E, [c], fused)
    y, extra, limited = _unlimited(res, 0)
    name = er.case_id(case)
    if c.mode == "std":
        name += " gated" if pipe.gated_used else " two-pass"
    if c.mode in ("std", "static_pad", "static_nopad"):
        assert limited == 0, "built without the limiter"
        assert c.mode != "std" or float(res.stream_peaks(0).max()) <= LIMIT
        _assert_peaks_are_the_samples(res, 0, res.output(0))
        extra = None
    _assert_bound(name, c, ref, y, extra)
    return pipe


@pytest.mark.parametrize("case", er.GATE_CASES, ids=er.case_id)
def test_gate_edge_samples(case):
    """GatePipeline: the fused gated 2048 kernel (2048/512, 2048/256), the
    4096 register kernel, the generic hop, the 4096/2048 cross-fade."""
    pipe = _single(case)
    assert pipe.gated_used == (case[5] == "gated 2048")


@pytest.mark.parametrize("case", [c for c in er.GATE_CASES if c[5] == "gated 2048" and c[3] == 2],
                         ids=er.case_id)
def test_gate_edge_samples_two_pass(case):
    """The same 2048 shapes through levels -> gate -> transform."""
    pipe = _single(case, fused=False)
    assert not pipe.gated_used


@pytest.mark.parametrize("case", er.ADAPTIVE_CASES, ids=er.case_id)
def test_adaptive_edge_samples(case):
    """AdaptivePipeline, norm "max": sum w^2 == 0 at sample 0, head and tail."""
    _single(case)


@pytest.mark.parametrize("case", er.STATIC_CASES, ids=er.case_id)
def test_static_edge_samples(case):
    """StaticEqPipeline with and without pad: 4096/2048 register kernel, three
    channels on the any-size path at 512/128, Bluestein 100/25, HBM 12000/3000."""
    _single(case)


# ---------------------------------------------------------------------------
# b. ragged batch in one launch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("batch", er.BATCHES, ids=er.batch_id)
def test_ragged_batch_edges(batch):
    """Three streams, one per tail class, packed in one launch: the tail of one
    lies directly before the head of the next, in the input and in the output.
    Every stream meets the bound and equals its own single-stream run bit for
    bit."""
    torch, E = _engine()
    ch, fused = batch[3], batch[5]
    cases = er.batch_cases(batch)
    refs = er.batch_references(batch)
    cs = [r[0] for r in refs]
    pipe, res = _run(torch, E, cs, fused)
    offs = list(res.out_offs)
    assert all(offs[i + 1] == offs[i] + res.out_lens[i] * ch for i in range(2)), "outputs packed"
    together = [res.output(i).copy() for i in range(3)]
    unl = [_unlimited(res, i) for i in range(3)]
    for i, c in enumerate(cs):
        y, extra, _ = unl[i]
        _assert_bound(f"{er.case_id(cases[i])} stream {i} of 3", c, refs[i], y,
                      None if c.mode in ("std", "static_pad", "static_nopad") else extra)
    for i, c in enumerate(cs):
        _, alone = _run(torch, E, [c], fused)
        assert np.array_equal(alone.output(0).view(np.uint32), together[i].view(np.uint32)), i
        assert np.array_equal(alone.stream_peaks(0).view(np.uint32),
                              res.stream_peaks(i).view(np.uint32)), i


# ---------------------------------------------------------------------------
# c. silent edges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("silent", er.SILENT, ids=er.batch_id)
def test_silent_edges_are_zero_and_unflagged(silent):
    """Digital silence over the first and last 2 n_fft samples, a loud middle
    (over the limit).  A frame that reaches an output sample of the first or
    last n_fft lies wholly inside the silence, so the device writes exact zeros
    there -- every ill-conditioned sample among them -- and the chunk's scale is
    determined: unflagged.  The rest of the stream meets the bound."""
    torch, E = _engine()
    mode, n_fft, hop, ch, path, fused = silent
    ref = er.silent_reference(silent)
    c, y64, s1, s2, D = ref
    case = c.case
    assert not c.x[:2 * n_fft].any() and not c.x[-2 * n_fft:].any() and c.x.any()
    pipe, res = _run(torch, E, [c], fused)
    y = res.output(0)
    assert not y[:n_fft].any() and not y[-n_fft:].any()
    assert not y64[:n_fft].any() and not y64[-n_fft:].any()
    edge = np.zeros(len(y), bool)
    edge[:n_fft] = edge[-n_fft:] = True
    assert (s2[~edge] >= cd.TAU).all(), "every ill-conditioned sample lies in the zero edges"
    yu, extra, limited = _unlimited(res, 0)
    _assert_bound(f"{er.case_id(case)} silent edges", c, ref, yu, extra)
    if mode == "static_pad":
        assert float(res.stream_peaks(0).max()) > 0.99
        assert res.scale_flags(0, limit=0.99) == [False]
    else:
        if mode != "adaptive":
            assert limited == 1, "the loud middle is over the limit"
        assert res.scale_flags(0) == [False] * len(res.chunk_ranges(0))


# ---------------------------------------------------------------------------
# d. / e. the peak and the limiter at an ill-conditioned sample (pe == 0)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("gains,flagged", [("tilt", True), ("random", False)])
@pytest.mark.parametrize("n_fft,hop,path", [(2048, 512, "gated 2048"), (4096, 1024, "4096")])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twopass"])
def test_peak_and_limiter_cover_the_edge(n_fft, hop, path, fused, gains, flagged):
    """pe == 0: the last frame ends at N and the largest sample of the stream is
    an ill-conditioned one.  Without the limiter (output gain 2^-24) the
    chunk's peak is that sample, bit for bit.  With it (the same run at output
    gain 1: every value 2^24 times larger, exactly) every sample of the chunk,
    the edge samples included, is float32(y * float32(0.999 / peak)) bit for
    bit.

    With the pipeline's own tilt rows (what every production run has) the
    filter's time-aliased tail is small, the edge sample a few tens, and the
    model's uncertainty of it about 1 %: the chunk is flagged.  With random
    per-bin gains that tail is 2e4 and the same uncertainty 1e-5 of it, below
    ETA: the scale is determined by an ill-conditioned sample, and unflagged
    (conditioning.chunk_flags on the float64 reference says the same)."""
    torch, E = _engine()
    case = ("std", n_fft, hop, 2, "tail0", path)
    own = gains == "tilt"
    c, _, s1, s2, _ = er.reference(case)
    pipe, res = _run(torch, E, [c], fused, own_gains=own)
    assert pipe.gated_used == (fused and path == "gated 2048")
    y_off = res.output(0).copy()
    assert res.chunk_ranges(0) == [(0, c.N)]
    _assert_peaks_are_the_samples(res, 0, y_off)
    p = int(np.abs(y_off).max(axis=1).argmax())
    assert s2[p] < cd.TAU and p >= c.N - n_fft, "the peak is an ill-conditioned tail sample"
    well = float(np.abs(y_off[s2 >= cd.TAU]).max())
    assert float(np.abs(y_off[p]).max()) > 4 * well
    assert float(res.stream_peaks(0)[0]) <= LIMIT
    assert res.scale_flags(0) == [False]   # under the limit: nothing to flag

    c_on = er.build(case, gain_log2=0)
    assert np.array_equal(c_on.x, c.x) and np.array_equal(c_on.gains, c.gains)
    pipe_on, res_on = _run(torch, E, [c_on], fused, own_gains=own)
    assert pipe_on.gated_used == pipe.gated_used
    k = np.float32(2.0 ** -er.STD_GAIN_LOG2)
    y_nolimit = y_off * k                              # exact: a power of two, no underflow
    assert np.array_equal(y_nolimit / k, y_off)
    peak = res_on.stream_peaks(0)
    assert peak.shape == (1,) and peak[0] == np.abs(y_nolimit).max() and peak[0] > LIMIT
    want = y_nolimit * (LIMIT / np.float32(peak[0]))
    got = res_on.output(0)
    assert got.dtype == want.dtype == np.float32
    print(f"EDGE PEAK {n_fft}/{hop} {'gated' if pipe.gated_used else 'two-pass'} {gains}: "
          f"peak {peak[0]:.6g} at {p} of {c.N}, sum w^2 {s2[p]:.3g}, well-conditioned max "
          f"{well * float(k):.4g}")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert res_on.scale_flags(0) == [flagged]


# ---------------------------------------------------------------------------
# f. a last frame that ends short of N (found by (a): plan_create refused it)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pipelined", [False, True], ids=["plain", "pipelined"])
def test_last_frame_short_of_n(ch, pipelined):
    """2048/300 with pe == 0: hop does not divide n_fft / 2, the last frame ends
    124 samples short of N and the reference writes 0 / (0 + 1e-12) there.  The
    engine used to hand the plan an output range beyond the last frame, which
    tomatis_plan_create refuses (124 of every 300 lengths at this shape).  With
    the limiter on (output gain 1), twice through the same pipeline (a pipelined
    one declines this shape and runs plain): N samples, exact zeros past the
    last frame, the bound everywhere else."""
    torch, E = _engine()
    case = ("std", 2048, 300, ch, "tail0", "generic hop")
    ref = er.reference(case, gain_log2=0)
    c, y64, s1, s2, D = ref
    end = c.geom["first_start"] + (c.geom["n_frames"] - 1) * c.hop + c.n_fft
    assert end == c.N - 124
    ss = E.StreamSet.from_arrays([c.x], SR)
    pipe = E.GatePipeline(ss, pipelined=pipelined, **c.params)
    _set_gains(torch, pipe, c.gains)
    first = None
    for _ in range(2):
        pipe.run()
        res = pipe.result()
        y = res.output(0).copy()
        assert y.shape == (c.N, ch) and not y[end:].any() and y[end - 300:end].any()
        assert np.array_equal(res.stream_states(0), c.oref["states"])
        assert first is None or np.array_equal(first.view(np.uint32), y.view(np.uint32))
        first = y
    assert res.chunk_ranges(0) == [(0, c.N)]   # one chunk: the zeros scale to zeros
    yu, extra, limited = _unlimited(res, 0)
    assert limited == 1
    _assert_bound(f"{er.case_id(case)} limiter on", c, ref, yu, extra)
