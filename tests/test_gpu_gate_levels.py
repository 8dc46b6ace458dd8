"""The gate scans on crafted levels against the sequential gate.

Every kernel group that restates one of the reference's gate loops is launched
alone on levels written straight into the pipeline's buffer (plans over zeros,
no audio), and compared exactly -- states and rows as integers, alpha as
float64 bit patterns -- with the oracle's loop on the same array:

* run-scan gate       tomatis_gate_std            (k_gate_sum / carry / states)
* transfer-table gate tomatis_gate_std, GATE_TF   (k_gate_tf / chain / resolve)
* cross-fade alpha    tomatis_gate_std, alpha 1   (k_alpha_sync / chain / prefix)
* host-carry entries  tomatis_gate_segment_sums, tomatis_gate_std_carry
* time shards         tomatis_ts_summary, tomatis_ts_gate (k_ts_fold / k_ts_carry)
* min-hold            tomatis_minhold_bisect      (k_mh_probe / k_minhold)

The sequences come from tests/gate_ref.py (what they hold is asserted on the
CPU in tests/test_gate_ref.py).  The truth is never the intended predicate: it
is the oracle's verdict on the float32 array the device gets.  One last case
goes through audio and the fused in-kernel gate."""
import functools

import numpy as np
import pytest

from oracle import tomatis_oracle as orc
from tests import gate_ref as G

pytestmark = pytest.mark.gpu

SR_SMALL = 16000      # 64 / 16 at 16 kHz: one frame per millisecond
SR_REG = 51200        # 2048 / 512 at 51.2 kHz: one frame per 10 ms


def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import engine
    return torch, engine


def _lib():
    from tomatis_audio_processor_amd import _lib
    return _lib


def _std_samples(F, n_fft, hop):
    """Samples giving F standard-mode frames (1 sample: no frame)."""
    return hop * (F - 1) + n_fft // 2 if F > 0 else 1


@functools.lru_cache(maxsize=None)
def _stream_set(shape):
    """Zero-filled streams (the levels are overwritten): ``ragged`` the mono
    64 / 16 streams of G.STREAM_FRAMES, ``register`` one stereo 2048 / 512
    stream, ``tiles`` one mono 64 / 16 stream of more than 256 segments."""
    _, E = _gpu()
    if shape == "ragged":
        return E.StreamSet.from_arrays([np.zeros((_std_samples(F, 64, 16), 1), np.float32)
                                        for F in G.STREAM_FRAMES], SR_SMALL)
    if shape == "register":
        return E.StreamSet.from_arrays(
            [np.zeros((_std_samples(G.F_REGISTER, 2048, 512), 2), np.float32)], SR_REG)
    if shape == "tiles":
        return E.StreamSet.from_arrays(
            [np.zeros((_std_samples(G.F_TILES, 64, 16), 1), np.float32)], SR_SMALL)
    raise ValueError(shape)


_FRAMES = {"ragged": G.STREAM_FRAMES, "register": (G.F_REGISTER,), "tiles": (G.F_TILES,)}


def _pipeline(shape, D, **kw):
    _, E = _gpu()
    ss = _stream_set(shape)
    if shape == "register":
        pipe = E.GatePipeline(ss, gate_ui=50, n_fft=2048, hop=512, up_delay_ms=10.0 * D, **kw)
    else:
        pipe = E.GatePipeline(ss, gate_ui=50, n_fft=64, hop=16, up_delay_ms=float(D), **kw)
    assert pipe.up_delay_frames == D
    assert tuple(s.n_frames for s in pipe.streams) == _FRAMES[shape]
    return pipe


@functools.lru_cache(maxsize=None)
def _rounds(shape, D, hyst, both=False):
    """The catalogue as rounds over a plan's streams: round j gives stream i its
    pattern j (mod its count), as float32 bit patterns drawn from the alphabet
    of these thresholds, with the oracle's states on exactly those arrays.
    Computed once per (shape, D, thresholds) and shared by the tests."""
    Ton, Toff = G.thresholds(hyst)
    ab = G.Alphabet(Ton, Toff)
    rng = np.random.default_rng(7919 * D + len(shape))
    if shape == "tiles":
        per = [[("tiled", G.tiled(G.F_TILES, D, rng=rng))]]
    else:
        per = [list(G.patterns(F, D, rng=rng, both=both)) for F in _FRAMES[shape]]
    out = []
    for j in range(max(len(p) for p in per)):
        bits = [ab.r_bits(p[j % len(p)][1], rng) for p in per]
        want = [G.oracle_states(b.view(np.float32), Ton, Toff, D) for b in bits]
        out.append(([p[j % len(p)][0] for p in per], bits, want))
    return out


def _flat(pipe, parts, dtype):
    out = np.zeros(max(1, pipe.plan.total_frames), dtype)
    for s, p in zip(pipe.streams, parts):
        out[s.frame_base:s.frame_base + s.n_frames] = p
    return out


def _upload_r(torch, pipe, bits):
    """float32 levels by bit pattern (NaN payloads and all)."""
    flat = _flat(pipe, bits, np.uint32)
    pipe.r.view(torch.int32)[:len(flat)].copy_(torch.from_numpy(flat.view(np.int32)))


def _gate_std(torch, pipe):
    L = _lib()
    pipe.states.zero_()
    pipe.rows.fill_(-1)
    if pipe.alpha is not None:
        pipe.alpha.fill_(-7.0)
    L.check(L.lib().tomatis_gate_std(pipe.plan.h, L.ptr(pipe.r), L.ptr(pipe.states),
                                     L.ptr(pipe.rows), L.ptr(pipe.alpha), L.stream_handle()),
            "gate_std")
    torch.cuda.synchronize()
    Ft = pipe.plan.total_frames
    return (pipe.states[:Ft].cpu().numpy(), pipe.rows[:Ft].cpu().numpy().view(np.uint16),
            None if pipe.alpha is None else pipe.alpha[:Ft].cpu().numpy())


def _is_run_scan(pipe):
    """The plan's gate form: tomatis_gate_segment_sums serves the run-scan form
    alone (TOMATIS_E_UNSUPPORTED under the transfer-table form)."""
    L = _lib()
    n = int(L.lib().tomatis_plan_gate_segments(pipe.plan.h))
    sums = np.zeros(5 * max(1, n), np.int32)
    rc = L.lib().tomatis_gate_segment_sums(pipe.plan.h, L.ptr(pipe.r), sums.ctypes.data,
                                           L.stream_handle())
    assert rc in (0, L.E_UNSUPPORTED), rc
    return rc == 0


def _check_states(torch, pipe, rounds, what):
    for names, bits, want in rounds:
        _upload_r(torch, pipe, bits)
        st, rows, _ = _gate_std(torch, pipe)
        ref = _flat(pipe, want, np.uint8)[:len(st)]
        if not np.array_equal(st, ref):
            k = int(np.nonzero(st != ref)[0][0])
            i = max(i for i, s in enumerate(pipe.streams) if s.frame_base <= k and s.n_frames)
            raise AssertionError(f"{what}: stream {i} ({pipe.streams[i].n_frames} frames), pattern "
                                 f"{names[i]}, frame {k - pipe.streams[i].frame_base}: state "
                                 f"{st[k]}, the oracle's {ref[k]}")
        assert np.array_equal(rows, ref.astype(np.uint16) - 1), (what, names)


# ---------------------------------------------------------------------------
# run-scan gate and transfer-table gate
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ragged", "register"])
@pytest.mark.parametrize("D", G.DELAYS)
def test_run_scan_gate_equals_the_oracle(D, shape):
    torch, _ = _gpu()
    pipe = _pipeline(shape, D, hysteresis_db=3.0)
    assert (pipe.Ton, pipe.Toff) == G.thresholds(3.0)
    assert _is_run_scan(pipe), "hysteresis 3 dB: no level is on and off, the run-scan form"
    _check_states(torch, pipe, _rounds(shape, D, 3.0), f"run-scan D={D}")


@pytest.mark.parametrize("shape", ["ragged", "register"])
@pytest.mark.parametrize("D", G.DELAYS)
def test_transfer_table_gate_equals_the_oracle_on_the_same_arrays(D, shape):
    torch, _ = _gpu()
    with _lib().dev_options(GATE_TF=1):
        pipe = _pipeline(shape, D, hysteresis_db=3.0)
        assert not _is_run_scan(pipe)
        _check_states(torch, pipe, _rounds(shape, D, 3.0), f"transfer table D={D}")


@pytest.mark.parametrize("hyst", [0.0, -2.0])
@pytest.mark.parametrize("D", G.DELAYS)
def test_transfer_table_gate_with_levels_that_are_on_and_off(D, hyst):
    """hysteresis <= 0: Ton <= Toff, levels between them are on and off at once
    (C1 treats them as on, C2 leaves on them); the plan picks the table form by
    itself."""
    torch, _ = _gpu()
    pipe = _pipeline("ragged", D, hysteresis_db=hyst)
    assert not _is_run_scan(pipe)
    rounds = _rounds("ragged", D, hyst, True)
    assert any((G.pred_of_r(b.view(np.float32), pipe.Ton, pipe.Toff) == G.BOTH).any()
               for _, bits, _ in rounds for b in bits)
    _check_states(torch, pipe, rounds, f"transfer table hysteresis={hyst} D={D}")


@pytest.mark.parametrize("D", G.DELAYS)
def test_gates_over_more_than_256_segments(D):
    """One stream of 257 segments and a bit: k_gate_carry's second tile, with an
    on-run that matures on the tile's first frame.  (The time goes to the
    oracle's Python loop over 2.6e5 frames.)"""
    torch, _ = _gpu()
    rounds = _rounds("tiles", D, 3.0)
    pipe = _pipeline("tiles", D, hysteresis_db=3.0)
    assert int(_lib().lib().tomatis_plan_gate_segments(pipe.plan.h)) > G.TILE
    assert _is_run_scan(pipe)
    _check_states(torch, pipe, rounds, f"run-scan, 257 segments, D={D}")
    del pipe
    with _lib().dev_options(GATE_TF=1):
        pipe = _pipeline("tiles", D, hysteresis_db=3.0)
        assert not _is_run_scan(pipe)
        _check_states(torch, pipe, rounds, f"transfer table, 257 segments, D={D}")


# ---------------------------------------------------------------------------
# host-carry entry points
# ---------------------------------------------------------------------------

def _carries(D, n):
    """Carries (a, e, f) a stream can start from: idle, a run pending for j
    frames (a = -1 - j), in C2 (last entry after the last off frame), back in
    C1 with a run pending."""
    from tomatis_audio_processor_amd.timeshard import NONE
    kinds = [(-1, NONE, NONE)]
    for j in (1, max(1, D - 1), D, D + 1, D + 2):
        kinds.append((-1 - j, NONE, NONE))
    kinds += [(-1 - (D + 1), -1, NONE), (-3, -3 - 7, -3 - 9), (-3, -3 - 9, -3), (-1 - D, -40 - D, -1 - D)]
    return [kinds[(i + D) % len(kinds)] for i in range(n)]


@pytest.mark.parametrize("D", G.DELAYS)
def test_segment_sums_and_gate_from_a_carry_equal_the_host_mirror(D):
    torch, _ = _gpu()
    from tomatis_audio_processor_amd import timeshard as T
    L = _lib()
    pipe = _pipeline("ragged", D, hysteresis_db=3.0)
    n_segs = int(L.lib().tomatis_plan_gate_segments(pipe.plan.h))
    assert n_segs == sum(-(-F // G.SEG) for F in G.STREAM_FRAMES)
    carries = _carries(D, len(pipe.streams))
    carry_host = np.asarray(carries, np.int32).reshape(-1)
    assert any(c != T.C1_IDLE for c in carries)
    rounds = _rounds("ragged", D, 3.0)
    for names, bits, _ in rounds:
        _upload_r(torch, pipe, bits)
        preds = [G.pred_of_r(b.view(np.float32), pipe.Ton, pipe.Toff) for b in bits]
        sums = np.full(5 * n_segs, 12345, np.int32)
        L.check(L.lib().tomatis_gate_segment_sums(pipe.plan.h, L.ptr(pipe.r), sums.ctypes.data,
                                                  L.stream_handle()), "segment_sums")
        want = [T.summarize(p[a:a + G.SEG], D, k0=a) for p in preds
                for a in range(0, len(p), G.SEG)]
        assert sums.reshape(-1, 5).tolist() == [list(map(int, w)) for w in want], names
        pipe.states.zero_()
        pipe.rows.fill_(-1)
        L.check(L.lib().tomatis_gate_std_carry(pipe.plan.h, L.ptr(pipe.r), carry_host.ctypes.data,
                                               L.ptr(pipe.states), L.ptr(pipe.rows),
                                               L.stream_handle()), "gate_std_carry")
        Ft = pipe.plan.total_frames
        st = pipe.states[:Ft].cpu().numpy()
        ref = _flat(pipe, [T.resolve(p, D, c) for p, c in zip(preds, carries)], np.uint8)[:Ft]
        assert np.array_equal(st, ref), names
        assert np.array_equal(pipe.rows[:Ft].cpu().numpy().view(np.uint16),
                              ref.astype(np.uint16) - 1), ("rows from a carry", names)


# ---------------------------------------------------------------------------
# time shards without the transform
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("D", G.DELAYS)
def test_time_shard_gate_equals_the_sequential_gate(D, world):
    torch, _ = _gpu()
    from tomatis_audio_processor_amd import timeshard as T
    L = _lib()
    F = G.F_SHARDED
    N = _std_samples(F, 64, 16)
    shards = T.plan_shards(N, 64, 16, world)
    assert len(shards) == world and shards[-1].k1 == F
    x = np.zeros((N, 1), np.float32)
    runners = [T.ShardRunner(x[s.lo:s.hi], SR_SMALL, s, ch=1, gate_ui=50, n_fft=64, hop=16,
                             hysteresis_db=3.0, up_delay_ms=float(D)) for s in shards]
    Ton, Toff = G.thresholds(3.0)
    assert all(rn.pipe.up_delay_frames == D and (rn.pipe.Ton, rn.pipe.Toff) == (Ton, Toff)
               for rn in runners)
    ab = G.Alphabet(Ton, Toff)
    rng = np.random.default_rng(31 * D + world)
    hs = L.stream_handle()
    for name, pred in G.shard_patterns(shards, F, D, rng):
        bits = ab.r_bits(pred, rng)
        r = bits.view(np.float32)
        verdict = G.pred_of_r(r, Ton, Toff)
        want = G.oracle_states(r, Ton, Toff, D)
        for rn in runners:                            # the shard's slice of the one global array
            s, n = rn.shard, rn.shard.geometry["n_frames"]
            assert rn.pipe.plan.total_frames == n
            rn.pipe.r.view(torch.int32)[:n].copy_(
                torch.from_numpy(bits[s.b:s.b + n].view(np.int32)))
            n_tf_segs = -(-s.tf_frames // G.SEG)
            L.check(L.lib().tomatis_ts_summary(rn.pipe.plan.h, L.ptr(rn.pipe.r), n_tf_segs, s.b,
                                               L.ptr(rn.sum5), hs), "ts_summary")
        sums_all = torch.cat([rn.sum5 for rn in runners])
        got5 = sums_all.cpu().numpy().reshape(-1, 5).tolist()
        want5 = [list(map(int, T.summarize(verdict[s.b:s.b + s.tf_frames], D, k0=s.b)))
                 for s in shards]
        assert got5 == want5, (name, got5, want5)
        sts = []
        for rn in runners:
            s, pp = rn.shard, rn.pipe
            pp.states.zero_()
            L.check(L.lib().tomatis_ts_gate(pp.plan.h, L.ptr(pp.r), L.ptr(sums_all), s.rank, -s.b,
                                            L.ptr(pp.states), L.ptr(pp.rows), hs), "ts_gate")
            sts.append(pp.states[s.k0 - s.b:s.k1 - s.b].cpu().numpy())
        got = np.concatenate(sts)
        assert len(got) == F
        if not np.array_equal(got, want):
            k = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"world {world}, D {D}, {name}: frame {k} state {got[k]}, the "
                                 f"sequential gate's {want[k]}")


# ---------------------------------------------------------------------------
# cross-fade alpha
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _xfade_rounds(xf, Ton, Toff):
    ab = G.Alphabet(Ton, Toff)
    rng = np.random.default_rng(100 + xf)
    per = [list(G.xfade_state_patterns(F, xf, rng)) for F in G.STREAM_FRAMES]
    out = []
    for j in range(max(len(p) for p in per)):
        bits = [ab.r_bits(p[j % len(p)][1], rng) for p in per]
        st = [G.oracle_states(b.view(np.float32), Ton, Toff, 0) for b in bits]
        al = [orc.alpha_scan_xfade(s, xf) for s in st]
        out.append(([p[j % len(p)][0] for p in per], bits, st, al, [G.xfade_rows(a, xf) for a in al]))
    return out


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("xf", G.XFADES)
def test_xfade_alpha_and_rows_equal_the_oracle(xf, seq):
    torch, E = _gpu()
    pipe = E.GatePipeline(_stream_set("ragged"), gate_ui=50, n_fft=64, hop=16, up_delay_ms=0.0,
                          hysteresis_db=3.0, xfade_ms=float(xf))
    assert pipe.xf == xf and pipe.up_delay_frames == 0 and pipe.alpha is not None
    with _lib().dev_options(ALPHA_SEQ=seq):
        for names, bits, st_w, al_w, rows_w in _xfade_rounds(xf, pipe.Ton, pipe.Toff):
            _upload_r(torch, pipe, bits)
            st, rows, al = _gate_std(torch, pipe)
            n = len(st)
            assert np.array_equal(st, _flat(pipe, st_w, np.uint8)[:n]), names
            want = _flat(pipe, al_w, np.float64)[:n]
            if not np.array_equal(al.view(np.uint64), want.view(np.uint64)):
                k = int(np.nonzero(al.view(np.uint64) != want.view(np.uint64))[0][0])
                i = max(i for i, s in enumerate(pipe.streams) if s.frame_base <= k and s.n_frames)
                raise AssertionError(f"xf {xf}, ALPHA_SEQ {seq}, {names[i]}, stream {i}, frame "
                                     f"{k - pipe.streams[i].frame_base}: alpha {al[k]!r}, the "
                                     f"oracle's {want[k]!r}")
            assert np.array_equal(rows, _flat(pipe, rows_w, np.uint16)[:n]), names


# ---------------------------------------------------------------------------
# min-hold
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _minhold_rounds(mh):
    """G.minhold_rounds with the oracle's threshold and states; shared by the
    cross-fade lengths."""
    out = []
    for _, lv in G.minhold_rounds(mh):
        t = [orc.optimal_threshold(v, v > -70, G.MH_HYST, mh, G.MH_TARGET) if len(v) else None
             for v in lv]
        st = [orc.gate_minhold(v, tt, G.MH_HYST, mh) if len(v) else np.zeros(0, np.uint8)
              for v, tt in zip(lv, t)]
        out.append((lv, t, st))
    return out


@pytest.mark.parametrize("xf", [0, 1, 24])
@pytest.mark.parametrize("mh", G.MINHOLDS)
def test_minhold_states_and_alpha_equal_the_oracle(mh, xf):
    """OPT_MINHOLD_SERIAL 1 and 0.  The plan does not tell which kernels 0
    runs: it builds the speculative probes only when every stream's transfer
    tables (segments x 2 (mh + 1) entries) fit the probe kernel's LDS.  With
    these streams that holds up to mh = 1023; from mh = 1024 on both values run
    the serial kernel, and the second run only repeats the first.  What the
    level arrays hold (the "jump" streams that keep the bisection going for all
    30 steps with the C2 share on both sides of the target, at every mh) is
    asserted on the CPU in tests/test_gate_ref.py."""
    torch, E = _gpu()
    L = _lib()
    ss = E.StreamSet.from_arrays([np.zeros((16 * (F + 1), 1), np.float32) for F in G.MH_FRAMES],
                                 SR_SMALL)
    pipe = E.AdaptivePipeline(ss, n_fft=64, hop=16, min_hold_ms=float(mh), xfade_ms=float(xf),
                              hyst_db=G.MH_HYST, target_c2=G.MH_TARGET)
    sts = pipe.plan.streams
    assert pipe.mh == mh and pipe.xf == xf
    assert tuple(sts[i].n_frames for i in range(len(G.MH_FRAMES))) == G.MH_FRAMES
    Ft, hs = pipe.plan.total_frames, L.stream_handle()
    for lv_w, t_w, st_w in _minhold_rounds(mh):
        lv = np.zeros(Ft, np.float64)
        for i, v in enumerate(lv_w):
            lv[sts[i].frame_base:sts[i].frame_base + len(v)] = v
        pipe.levels[:Ft].copy_(torch.from_numpy(lv))
        L.check(L.lib().tomatis_level_stats(pipe.plan.h, L.ptr(pipe.levels), L.ptr(pipe._tlh), hs),
                "level_stats")
        for serial in (1, 0):
            pipe.plan.set_option(L.OPT_MINHOLD_SERIAL, serial)
            pipe.states.zero_()
            pipe.rows.fill_(-1)
            pipe.alpha.fill_(-7.0)
            pipe.t_out.fill_(float("nan"))
            L.check(L.lib().tomatis_minhold_bisect(pipe.plan.h, L.ptr(pipe.levels), L.ptr(pipe._tlh),
                                                   pipe.target_c2, pipe.hyst_db, L.ptr(pipe.t_out),
                                                   L.ptr(pipe.states), L.ptr(pipe.rows),
                                                   L.ptr(pipe.alpha), hs), "minhold_bisect")
            torch.cuda.synchronize()
            t = pipe.t_out.cpu().numpy()
            st = pipe.states[:Ft].cpu().numpy()
            al = pipe.alpha[:Ft].cpu().numpy()
            rows = pipe.rows[:Ft].cpu().numpy().view(np.uint16)
            for i, F in enumerate(G.MH_FRAMES):
                if F == 0:
                    continue
                a, what = sts[i].frame_base, (mh, xf, serial, i, F)
                assert float(t[i]) == float(t_w[i]), (what, t[i], t_w[i])
                assert np.array_equal(st[a:a + F], st_w[i]), what
                want = orc.alpha_scan_adaptive(st_w[i], xf)
                assert np.array_equal(al[a:a + F].view(np.uint64), want.view(np.uint64)), what
                # rows of the adaptive table: 2 + m at alpha = m / xf (no pure rows)
                xfe = max(1, xf)
                assert np.array_equal(rows[a:a + F], 2 + np.rint(want * xfe).astype(np.uint16)), what


# ---------------------------------------------------------------------------
# one case through audio: the fused in-kernel gate, the two-pass chain, the oracle
# ---------------------------------------------------------------------------

def test_fused_gate_two_pass_chain_and_oracle_agree_on_audio():
    """RUN_FRAMES 48 and 131.  A pass whose in-kernel gate gives up its
    look-back re-runs on the two-pass chain (gate_fallbacks, printed, not
    asserted zero); at least one of the two values must end on the fused gate,
    or its states were never compared."""
    torch, E = _gpu()
    sr, D, x, r, _, states = G.audio_case()
    ss = E.StreamSet.from_arrays([x], sr)
    r_bits = np.asarray(r, np.float32).view(np.uint32)
    fused = []
    for run_frames in (48, 131):
        with _lib().dev_options(RUN_FRAMES=run_frames):
            two = E.GatePipeline(ss, gate_ui=50, n_fft=2048, hop=512, fused_levels=False)
            res2 = two.run()
            assert not two.gated_used and two.up_delay_frames == D
            st2, r2 = res2.stream_states(0), res2.stream_r(0)
            pipe = E.GatePipeline(ss, gate_ui=50, n_fft=2048, hop=512)
            res = pipe.run()
            torch.cuda.synchronize()
            print(f"RUN_FRAMES={run_frames}: gated_used={pipe.gated_used} "
                  f"gate_fallbacks={pipe.gate_fallbacks}")
            assert pipe.gated_used or pipe.gate_fallbacks == 1
            fused.append(pipe.gated_used)
            st, rr = res.stream_states(0), res.stream_r(0)
        assert np.array_equal(r2.view(np.uint32), r_bits), run_frames
        assert np.array_equal(rr.view(np.uint32), r_bits), run_frames
        assert np.array_equal(st2, states), f"RUN_FRAMES={run_frames}: two-pass chain, oracle"
        assert np.array_equal(st, states), f"RUN_FRAMES={run_frames}: fused gate, oracle"
    assert any(fused), "neither run ended on the fused gate: its states were not compared"
