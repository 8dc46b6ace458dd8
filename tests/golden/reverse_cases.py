"""Cases of the parameter-recovery goldens (tools/make_reverse_goldens.py), shared
by the tool and the tests.  A fixture holds no audio.  x is regenerated from a
seed as ``verify_cases.make_x`` does: the synthetic noise re-enveloped, here by
``quiet`` dB where the stream is at -60 dBFS and by ``loud`` dB where it is at
-20 dBFS (alternating halves of its 3 s period), then sent through a one-pole
low-pass (``pole``) at the same overall RMS.  The low-pass is needed: both
scripts take their spectra of the power mono sqrt(0.5 (L^2 + R^2)), a
rectified signal, and on white noise the rectifier's difference tones fill the
low band so that a C2 frame (-15 dB low, +15 dB high) shows a tilt near 0 dB and
no frame ever exceeds +5 dB; with a programme whose energy lies low, as music's
does, C1 frames come out near -27 dB and C2 frames between +11 and +20 dB.
y is the repository's CPU oracle (``process_standard``, linear gate at T = -40 dBFS, hysteresis 1 dB, no up-delay, +-``gain`` dB tilt) applied to x and
then shifted by ``shift`` samples: positive = the recording starts later (zeros
in front), negative = its first samples are lost.

Both reference scripts fix SR = 48000, N_FFT = 4096 and HOP = 2048 and estimate
the delay on a 2 kHz envelope, so an estimated delay is a multiple of 24: the
cut they make can never move a frame off 16-byte alignment, whatever the shift.
(tests/test_gpu_reverse.py runs the kernels on odd cuts directly.)"""
import functools

import numpy as np

SR, N_FFT, HOP = 48000, 4096, 2048
T_DBFS, HYST = -40.0, 1.0
GATE_OFFSET = -90.0          # linear gate: 1.0 * 50 + (-90) = -40 dBFS
DECIM = 997                  # the fixture keeps y[::DECIM]

# branches: p1201 / m5003: a positive and a negative odd shift, clear C1 / C2
# separation, both level classes > 10 frames, empty level bins; flat: no frame
# beyond +-5 dB ("无法估计Gate阈值"); one_class: no frame under -45 dBFS, so
# verify_tilt_amplitude prints its two count lines only
CASES = [
    dict(name="reverse_p1201", seed=321, sec=8, loud=-5.0, quiet=10.0, gain=15.0, shift=1201, pole=0.98),
    dict(name="reverse_m5003", seed=322, sec=7, loud=-5.0, quiet=10.0, gain=15.0, shift=-5003, pole=0.98),
    dict(name="reverse_flat", seed=323, sec=6, loud=-5.0, quiet=10.0, gain=1.5, shift=0, pole=0.98),
    dict(name="reverse_one_class", seed=324, sec=6, loud=-5.0, quiet=18.0, gain=15.0, shift=480, pole=0.98),
]
BY_NAME = {c["name"]: c for c in CASES}


def make_x(c):
    from tomatis_audio_processor_amd.synth import synth_stream
    n = SR * c["sec"] + 777
    x = synth_stream(c["seed"], n, 2, SR).reshape(n, 2)
    ph = np.arange(n) % (3 * SR)
    g = np.where((ph >= SR // 100) & (ph < (3 * SR) // 2),
                 np.float32(10.0 ** (c["quiet"] / 20)),
                 np.float32(10.0 ** (c["loud"] / 20))).astype(np.float32)
    x = (x * g[:, None]).astype(np.float32)
    from scipy.signal import lfilter
    p = float(c["pole"])
    lp = lfilter([1.0 - p], [1.0, -p], x.astype(np.float64), axis=0)
    lp *= np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(lp ** 2))
    return np.ascontiguousarray(lp, np.float32)


@functools.lru_cache(maxsize=None)
def _pair(name):
    from oracle import tomatis_oracle as orc
    c = BY_NAME[name]
    x = make_x(c)
    g = c["gain"]
    ref = orc.process_standard(x, SR, gate_ui=50, gate_mode="linear", gate_scale=1.0,
                               gate_offset=GATE_OFFSET, hysteresis_db=HYST, c1_low=g,
                               c1_high=-g, c2_low=-g, c2_high=g, up_delay_ms=0.0,
                               n_fft=N_FFT, hop=HOP)
    y = np.ascontiguousarray(ref["y"], np.float32).reshape(len(x), 2)
    d = c["shift"]
    if d > 0:
        y = np.concatenate([np.zeros((d, 2), np.float32), y])
    elif d < 0:
        y = y[-d:]
    y = np.ascontiguousarray(y, np.float32)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def make_pair(c):
    """-> (x, y); computed once per case, read-only."""
    return _pair(c["name"])
