"""GPU: the batch pipeline's hand-offs between UNLIKE batches, as batch.py
produces them (``run(check_device=False, prev_pipe=prev)``, then ``finish()`` /
``result()`` on the predecessor): AdaptiveGroups <-> AdaptivePipeline (a batch of
4 or more files, then a remainder of 1 to 3), a successor none of whose streams
has a frame (it launches nothing, so it cannot limit its predecessor in its
launch), an AdaptiveGroups one of whose groups has no frame, and a successor
with one frame (nearly all of the predecessor's runs have no partner run).

Every batch's output and chunk peaks equal the same batch run alone,
unpipelined, bit for bit (the limiter is the float32 ``limit / peak`` multiply
of src/process_tomatis.py:331-357 and process_tomatis_adaptive.py:340-345
wherever it runs).  Every predecessor with full-length streams has a chunk
over the limit (asserted from the standalone peaks), so a hand-off that limits
nothing cannot pass.  The limiter stays inside the successor's launch wherever
a launch exists: the flushes of pending passes during each hand-off are
counted.
"""
import numpy as np
import pytest

from tomatis_audio_processor_amd.synth import synth_stream

pytestmark = pytest.mark.gpu

LIMIT = np.float32(0.999)
CH = 2
GATE_KW = {
    "standard": dict(gate_ui=50),
    "xfade": dict(gate_ui=50, gate_offset=-90, xfade_ms=500.0),
}
# stream lengths in seconds and input gains per batch kind (1.0 / 1.4: limited,
# 0.2: not); the lengths get a few odd samples each
G_SECS, G_GAINS = [2.0, 3.1, 2.4, 4.0, 2.2, 5.0], [1.0, 0.2, 1.4, 1.4, 0.2, 1.0]
S_SECS, S_GAINS = [3.0, 2.0], [1.4, 0.2]
N_SECS, N_GAINS = [5.0, 2.0, 3.3], [1.0, 0.2, 1.4]


def _engine():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import engine
    return torch, engine


def _arrays(kind, seed, sr, n_fft, adaptive):
    """The streams of one batch: G (6 streams -> two groups), S (2 streams), N
    (3 streams), Z (one stream without a frame), T (one stream of n_fft / 2
    samples: the fewest frames the schedules give, one), H (a loud stream and
    three without a frame -> two groups, the second one without a frame)."""
    if kind == "Z":
        lens, gains = [1000 if adaptive else 300], [1.0]
    elif kind == "H":
        lens, gains = [3 * sr + 11, 200, 300, 400], [1.4, 1.0, 1.0, 1.0]
    elif kind == "T":
        lens, gains = [n_fft // 2], [1.0]
    else:
        secs, gains = {"G": (G_SECS, G_GAINS), "S": (S_SECS, S_GAINS), "N": (N_SECS, N_GAINS)}[kind]
        lens = [int(s * sr) + 7 * i + seed % 5 for i, s in enumerate(secs)]
    return [synth_stream(seed + i, n, CH, sr) * np.float32(g)
            for i, (n, g) in enumerate(zip(lens, gains))]


def _make(E, mode, kind, ss, n_fft, hop, pipelined):
    """The pipeline batch.py builds for this batch (batch._make_pipe)."""
    kw = dict(n_fft=n_fft, hop=hop)
    if mode != "adaptive":
        return E.GatePipeline(ss, pipelined=pipelined, second_buffer=False, **GATE_KW[mode], **kw)
    if kind in "GH":
        return E.AdaptiveGroups(ss, groups=2, pipelined=pipelined, second_buffer=False, **kw)
    return E.AdaptivePipeline(ss, pipelined=pipelined, second_buffer=False, **kw)


def _members(pipe):
    return list(getattr(pipe, "pipes", [pipe]))


def _over_limit(torch, peaks) -> bool:
    return bool((peaks.view(torch.float32) > float(LIMIT)).any())


def _final(res):
    """(output floats of the streams, chunk peaks) of a Result"""
    n = int(sum(res.out_lens)) * res.ch
    return res.y[:n], res.chunk_peaks


class _FlushCount:
    """AdaptivePipeline.flush / GatePipeline.flush wrapped: the pipelines whose
    flush was entered with a pass pending."""

    def __init__(self, monkeypatch, E):
        self.hits = []
        for cls in (E.AdaptivePipeline, E.GatePipeline):
            orig = cls.flush

            def flush(pipe, _orig=orig):
                if pipe.pending:
                    self.hits.append(pipe)
                return _orig(pipe)
            monkeypatch.setattr(cls, "flush", flush)


def _run_chain(monkeypatch, mode, kinds, n_fft=2048, hop=512, sr=44100):
    torch, E = _engine()
    adaptive = mode == "adaptive"
    sss, refs = [], []
    for b, kind in enumerate(kinds):
        ss = E.StreamSet.from_arrays(_arrays(kind, 4100 + 37 * b, sr, n_fft, adaptive), sr)
        sss.append(ss)
        alone = _make(E, mode, kind, ss, n_fft, hop, pipelined=False)
        res = alone.run()
        y, pk = _final(res)
        refs.append(dict(y=y.clone(), pk=pk.clone(), out_lens=list(res.out_lens)))
        if kind not in "ZT":
            # precondition: something to limit, in every group of the batch
            for g, p in enumerate(_members(alone)[:1 if kind == "H" else None]):
                assert _over_limit(torch, p.peaks), f"batch {b} ({kind}) group {g}: no chunk over the limit"
        del alone, res
    counter = _FlushCount(monkeypatch, E)

    def check(b, pipe):
        """batch b's output is final: batch.py's store() (the last batch has no
        successor: its result() flushes it)"""
        if b + 1 < len(kinds):
            assert not pipe.pending, f"batch {b} ({kinds[b]}) still pending after its successor's run"
        pipe.finish()
        res = pipe.result()
        y, pk = _final(res)
        assert res.out_lens == refs[b]["out_lens"]
        assert torch.equal(pk, refs[b]["pk"]), f"batch {b} ({kinds[b]}): chunk peaks differ"
        assert torch.equal(y, refs[b]["y"]), f"batch {b} ({kinds[b]}): output differs"
        if kinds[b] == "Z":
            assert res.out_lens == [sss[b].lens[0] if adaptive else 0]
            assert not res.output(0).any(), "a stream without a frame: zeros"
            if adaptive:
                assert np.isnan(res.extra["thresholds"].cpu().numpy()).all()

    prev = None
    for b, (kind, ss) in enumerate(zip(kinds, sss)):
        pipe = _make(E, mode, kind, ss, n_fft, hop, pipelined=True)
        waiting = [p for p in _members(prev) if p.pending] if prev is not None else []
        counter.hits.clear()
        pipe.run(check_device=False, prev_pipe=prev)
        hits = list(counter.hits)
        where = f"{kinds[b - 1] if b else '-'} -> {kind} (batch {b})"
        if prev is not None:
            check(b - 1, prev)
        if kind == "Z":
            # nothing launched: every pending member is limited on its own plan, once
            assert sorted(map(id, hits)) == sorted(map(id, waiting)), where
        elif kind == "H":
            # group 0 limits its partner inside its launch; group 1 launches
            # nothing: it flushes its partner, and the groups stop pipelining
            # together (group 0's own pass is limited at once)
            assert not pipe.pending and not pipe.pipelined, where
            assert sorted(map(id, hits)) == sorted(map(id, waiting[1:2] + pipe.pipes[:1])), where
        else:
            assert pipe.pending and pipe.pipelined, where
            if b and kinds[b - 1] == "G" and kind != "G":
                # one partner per launch: group 0 inside it, group 1 on its own plan
                assert len(hits) == 1 and hits[0] is prev.pipes[1], where
            else:
                assert hits == [], where
        prev = pipe
    check(len(kinds) - 1, prev)


@pytest.mark.parametrize("kinds", ["GSGSZS", "GZG", "STG", "ZG", "GHS"])
def test_adaptive_handoffs(monkeypatch, kinds):
    """AdaptiveGroups (G) and AdaptivePipeline (S, Z, T) batches in the orders
    batch.py produces: G -> S limits group 0 inside S's launch and flushes group
    1; a batch without a frame (Z) flushes what is pending and is final at once,
    first in the chain too; a one-frame batch (T) limits a long predecessor in
    the follow-up launch; an AdaptiveGroups whose second group has no frame (H)
    keeps the in-launch hand-off for its first group."""
    _run_chain(monkeypatch, "adaptive", list(kinds))


@pytest.mark.parametrize("mode,kinds,shape", [
    ("standard", "NZNTN", (2048, 512, 44100)),
    ("xfade", "NZN", (2048, 512, 44100)),
    ("xfade", "NZN", (4096, 1024, 96000)),
])
def test_gate_handoffs(monkeypatch, mode, kinds, shape):
    """GatePipeline batches (the fused gate at 2048 / 512; the two-pass chain
    for the cross-fade) around a 300-sample batch without a frame and a
    one-frame batch."""
    n_fft, hop, sr = shape
    _run_chain(monkeypatch, mode, list(kinds), n_fft=n_fft, hop=hop, sr=sr)


@pytest.mark.parametrize("entry", ["rows", "gated"])
def test_abi_no_frame_successor(entry):
    """tomatis_stft_ola_pipelined_after / tomatis_stft_ola_gated_pipelined_after
    called with a plan without a frame and a loud batch's pending output: either
    TOMATIS_E_UNSUPPORTED with prev_y untouched, or TOMATIS_OK with prev_y
    limited -- never TOMATIS_OK with prev_y as it was."""
    torch, E = _engine()
    from tomatis_audio_processor_amd._lib import E_UNSUPPORTED, lib, ptr, stream_handle
    mode = "adaptive" if entry == "rows" else "standard"
    sr, n_fft, hop = 44100, 2048, 512
    ss = E.StreamSet.from_arrays(_arrays("S", 4300, sr, n_fft, mode == "adaptive"), sr)
    ref = _make(E, mode, "S", ss, n_fft, hop, pipelined=False).run()
    assert _over_limit(torch, ref.chunk_peaks)
    loud = _make(E, mode, "S", ss, n_fft, hop, pipelined=True)
    assert loud.run() is None and loud.pending
    torch.cuda.synchronize()
    before = loud.y.clone()
    assert torch.equal(loud.peaks, ref.chunk_peaks) and not torch.equal(before, ref.y)
    zs = E.StreamSet.from_arrays(_arrays("Z", 4400, sr, n_fft, mode == "adaptive"), sr)
    z = _make(E, mode, "Z", zs, n_fft, hop, pipelined=False)
    z.run()                      # (its per-frame arrays as a pass leaves them)
    zy, zpk = torch.zeros_like(z.y), torch.zeros_like(z.peaks)
    L, hs = lib(), stream_handle()
    if entry == "rows":
        rc = L.tomatis_stft_ola_pipelined_after(
            z.plan.h, ptr(zs.x), ptr(z.gains), z.n_rows, ptr(z.rows), ptr(zy), ptr(zpk),
            float(LIMIT), loud.plan.h, ptr(loud.y), ptr(loud.peaks), hs)
    else:
        assert L.tomatis_gate_lookback(z.plan.h, ptr(zs.x), hs) == 0
        rc = L.tomatis_stft_ola_gated_pipelined_after(
            z.plan.h, ptr(zs.x), ptr(z.gains), z.n_rows, ptr(zy), ptr(zpk), float(LIMIT),
            ptr(z.r), ptr(z.states), loud.plan.h, ptr(loud.y), ptr(loud.peaks), hs)
    torch.cuda.synchronize()
    assert rc in (0, E_UNSUPPORTED), rc
    if rc == E_UNSUPPORTED:
        assert torch.equal(loud.y, before), "declined, yet prev_y was written"
        res = loud.result()      # the caller's part: the limiter on prev_plan
        assert torch.equal(res.y, ref.y)
    else:
        assert torch.equal(loud.y, ref.y), "TOMATIS_OK with prev_y left unlimited"
        loud.pending = False
