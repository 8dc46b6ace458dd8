"""Cases of the rational-ratio delay goldens (tools/make_rational_goldens.py):
pairs at 44.1 kHz, 88.2 kHz and 192 kHz, built as tests/golden/align_cases.py
builds its pairs (one synth stream, the target ``shift`` samples later,
attenuated, tilted and mixed with a second stream), 12 s against the middle
2 s with lengths that are no multiple of anything.  Every pair's float64
correlation, "valid" (layer2_analyze_eq) and "full" (compare_audio), keeps
its top >= MIN_MARGIN clear of the runner-up.  176.4 kHz has no delay golden:
the pair tried (seed 175) had a margin of 3.8e-5; its ratio 5 / 441 is covered
by the envelope tests."""
import numpy as np

MIN_MARGIN = 1e-3
DS_SR = 2000
CHUNK_SEC = 2


def _case(sr, shift, seed):
    sign = "p" if shift >= 0 else "m"
    return dict(name=f"rational_{sr}_{sign}{abs(shift)}", sr=sr, seed=seed, n_base=12 * sr + 7,
                n_target=12 * sr + 13, shift=shift, chunk_sec=CHUNK_SEC)


RATIONAL_CASES = [
    _case(44100, 1234, 171),
    _case(44100, -5003, 172),
    _case(88200, 2477, 173),
    _case(192000, -9001, 174),
]


def make_pair(c):
    """-> (target, base) float32 [n, 2]; the target is compare_audio's candidate."""
    from tomatis_audio_processor_amd.synth import synth_stream
    sr = c["sr"]
    offset = 5 * sr          # >= every |shift|
    base = synth_stream(c["seed"], c["n_base"], 2, sr, start=offset)
    u = synth_stream(c["seed"], c["n_target"] + 1, 2, sr, start=offset - c["shift"] - 1)
    other = synth_stream(c["seed"] + 1000, c["n_target"], 2, sr)
    tgt = np.float32(0.7) * u[1:] + np.float32(0.2) * u[:-1] + np.float32(0.05) * other
    return tgt.astype(np.float32), base
