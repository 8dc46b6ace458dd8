"""Cases of the alignment / layer-2 analysis goldens (tools/make_align_goldens.py):
inputs are regenerated from seeds.  A pair is cut from one synth stream: the
base starts at OFFSET, the target ``shift`` samples earlier in the stream (so
it plays the same material ``shift`` samples later), attenuated, tilted by a
two-tap filter and mixed with a second, quieter stream."""
import numpy as np

SR = 48000
OFFSET = 240000          # >= every |shift|

# find_delay: 12 s against the middle 2 s, except where a length says otherwise
DELAY_CASES = [
    dict(name="align_p1234", seed=71, n_base=12 * SR, n_target=12 * SR, shift=1234,
         chunk_sec=2),
    dict(name="align_m5000", seed=72, n_base=12 * SR, n_target=12 * SR, shift=-5000,
         chunk_sec=2),
    # lengths that are no multiple of the decimation (24)
    dict(name="align_p100007", seed=73, n_base=12 * SR + 7, n_target=12 * SR + 13,
         shift=100007, chunk_sec=2),
    # base shorter than the chunk: s, e clamp to the file
    dict(name="align_short_base", seed=74, n_base=72001, n_target=12 * SR, shift=30011,
         chunk_sec=2),
    # target shorter than the chunk: fftconvolve swaps its operands (host path)
    dict(name="align_short_target", seed=75, n_base=12 * SR, n_target=48011, shift=-250000 + 17,
         chunk_sec=2),
]

# the CLI: 40 s (longer than the default 25 s chunk)
CLI_CASES = [
    dict(name="align_cli_default", seed=81, n_base=40 * SR, n_target=40 * SR + 5, shift=777,
         argv=[]),
    dict(name="align_cli_2048", seed=82, n_base=40 * SR + 11, n_target=40 * SR, shift=-3210,
         argv=["--n_fft", "2048", "--hop", "1024", "--smooth_bins", "31", "--clamp_db", "6"]),
]

# the reference's two error paths
ERROR_CASES = [
    dict(name="align_err_overlap", seed=91, n_base=4800, n_target=4800, shift=0, argv=[]),
    dict(name="align_err_frames", seed=81, n_base=40 * SR, n_target=40 * SR + 5, shift=777,
         argv=["--music_dbfs", "10"]),
]


def make_pair(c):
    """-> (target, base) float32 [n, 2]."""
    from tomatis_audio_processor_amd.synth import synth_stream
    base = synth_stream(c["seed"], c["n_base"], 2, SR, start=OFFSET)
    u = synth_stream(c["seed"], c["n_target"] + 1, 2, SR, start=OFFSET - c["shift"] - 1)
    other = synth_stream(c["seed"] + 1000, c["n_target"], 2, SR)
    tgt = np.float32(0.7) * u[1:] + np.float32(0.2) * u[:-1] + np.float32(0.05) * other
    return tgt.astype(np.float32), base
