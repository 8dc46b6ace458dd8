"""GPU: the n_fft-2048 interior frame loop (k_stft_ola's fast_run) on small
streams cut into long runs, so that one interior run walks several limiter
chunks, stores its frames' r / states through its per-run pointers and --
pipelined -- rescales the partner pieces that its LDS-DMA brought in.

TOMATIS_DEV_SLOTS leaves one or a few run slots for the interior frames, so the
plan cuts runs of up to 4096 frames (tm_plan.cpp build_runs): 20 to 45 s of
audio against the limiter's 10 s chunks.  Loud input (sample peak 1.5: most
chunk peaks above the 0.999 limit) gives nearly every frame of a pipelined pass
a partner piece.  Every pipelined pass must equal an unpipelined pass over the
same input bit for bit (output, chunk peaks, r, states), and the fused gate
must equal the two-pass chain (tomatis_levels -> tomatis_gate_std ->
tomatis_stft_ola_limited) bit for bit, with no error bit and no fallback.
"""
import numpy as np
import pytest

from tomatis_audio_processor_amd.synth import synth_stream

pytestmark = pytest.mark.gpu
LIM = 0.999
SR = 44100


def _engine():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import engine
    return torch, engine


def _loud(E, lens, ch, seed0):
    """seeded streams of the given lengths, each scaled to a sample peak of 1.5"""
    xs = []
    for i, n in enumerate(lens):
        x = synth_stream(seed0 + i, n, ch, SR)
        xs.append(x * np.float32(1.5 / np.abs(x).max()))
    return E.StreamSet.from_arrays(xs, SR)


@pytest.mark.parametrize("case", [
    # (name, stream lengths, ch, hop, run slots)
    # one stream, two interior runs of ~30 s: three chunks per run
    ("stereo", [SR * 60 + 391], 2, 512, 3),
    # hop 256: two runs of ~3900 frames (22 s)
    ("mono_hop256", [SR * 45], 1, 256, 3),
    # ragged batch: interior runs of different lengths between edge runs, one
    # stream too short for an interior run
    ("ragged", [SR * 25 + 77, SR * 8 + 1, 3000, SR * 13], 2, 512, 9),
])
def test_interior_runs_over_several_chunks(case):
    torch, E = _engine()
    from tomatis_audio_processor_amd._lib import dev_options
    _, lens, ch, hop, slots = case
    kw = dict(gate_ui=50, n_fft=2048, hop=hop)
    with dev_options(SLOTS=slots):
        sets = [_loud(E, lens, ch, 4100 + 97 * j) for j in range(2)]
        ss = sets[0]
        xs = [sets[0].x, sets[1].x, sets[0].x]
        # the two-pass chain, then unpipelined fused passes over both inputs
        two = E.GatePipeline(ss, fused_levels=False, **kw)
        two.run()
        assert not two.gated_used
        ref = E.GatePipeline(ss, **kw)
        F = ref.plan.total_frames
        refs = []
        for x in xs[:2]:
            ref.ss.x = x
            ref.run()
            assert ref.gated_used and ref.gate_fallbacks == 0
            assert ref.plan.error_bits() == 0
            refs.append((ref.y.clone(), ref.peaks.clone(), ref.r.clone(), ref.states.clone()))
        y, pk, r, st = refs[0]
        assert float((pk.view(torch.float32) > LIM).float().mean()) > 0.5, "most chunks are loud"
        assert torch.equal(st[:F], two.states[:F]), "gate states differ from the two-pass chain"
        assert torch.equal(r[:F].view(torch.int32), two.r[:F].view(torch.int32)), "r differs"
        assert torch.equal(pk, two.peaks), "chunk peaks differ from the two-pass chain"
        assert torch.equal(y, two.y), "output differs from the two-pass chain"
        del two, ref
        # pipelined: pass k's output is final after pass k + 1 (or the flush)
        pipe = E.GatePipeline(ss, pipelined=True, **kw)
        got, cur = [], None
        for x in xs:
            pipe.ss.x = x
            assert pipe.run(check_device=False) is None and pipe.pending and pipe.pipelined
            if cur is not None:
                got.append((cur[0].clone(), cur[1].clone()) + cur[2:])
            cur = (pipe.y, pipe.peaks, pipe.r.clone(), pipe.states.clone())
        res = pipe.result()
        got.append((res.y, res.chunk_peaks) + cur[2:])
        assert pipe.finish() == 0 and not pipe.pending
        assert pipe.gate_fallbacks == 0
        for k, (y, pk, r, st) in enumerate(got):
            ry, rpk, rr, rst = refs[k % 2]
            assert torch.equal(st[:F], rst[:F]), f"pass {k}: states differ"
            assert torch.equal(r[:F].view(torch.int32), rr[:F].view(torch.int32)), f"pass {k}: r"
            assert torch.equal(pk, rpk), f"pass {k}: chunk peaks differ"
            assert torch.equal(y, ry), f"pass {k}: output differs"
