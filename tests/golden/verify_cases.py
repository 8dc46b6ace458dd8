"""Cases of the acceptance-validator goldens (tools/make_verify_goldens.py),
shared by the tool and the tests.  Inputs are regenerated from seeds: x is the
synthetic noise re-enveloped to -30 / -50 dBFS halves (as
tests/test_gpu_validator.py does), y the oracle's ``process_standard`` output
with a linear gate at T = -40 dBFS, hysteresis 1 dB, no up-delay: +-15 dB for
``verify_tomatis_15db_v2`` and +-5 dB for ``validate_layer1``.

The argparse defaults of the two reference CLIs are listed here as data
(``V2_DEFAULTS`` / ``L1_DEFAULTS``: flag -> value), so no test reads them from
the reference tree."""
import functools

import numpy as np

SR = 48000
N = SR * 12 + 777
T_DBFS, HYST = -40.0, 1.0
GATE_OFFSET = -90.0          # linear gate: 1.0 * 50 + (-90) = -40 dBFS
DECIM = 997                  # the fixture keeps y[::DECIM]

V2_DEFAULTS = dict(hyst_db=1.0, up_delay_ms=0, target_c2=0.5, fc=1000, slope=12, c1_low=15.0,
                   c1_high=-15.0, c2_low=-15.0, c2_high=15.0, n_fft=4096, hop=2048,
                   level_percentile=10, out_prefix="verify_15db_v2")
L1_DEFAULTS = dict(gate_ui=50, gate_scale=1.0, gate_offset=-61.08, hyst_db=1.0, up_delay_ms=0,
                   fc=1000, slope=12, c1_low=5.0, c1_high=-5.0, c2_low=-5.0, c2_high=5.0,
                   n_fft=4096, hop=2048, out_csv="layer1_spectrum_check.csv",
                   out_png="layer1_spectrum_check.png")

# x: kind "env" (re-enveloped), "loud" (the synthetic stream as it is), "silent";
# y: the oracle's output at +-gain dB, then "dc" (+0.002), "short" (one sample cut)
V2_CASES = [
    dict(name="verify_v2_st_4096", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=15.0),
    dict(name="verify_v2_mono_2048", seed=302, ch=1, n_fft=2048, hop=512, x="env", gain=15.0),
    dict(name="verify_v2_st_3000", seed=303, ch=2, n_fft=3000, hop=750, x="env", gain=15.0),
    dict(name="verify_v2_dc", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=15.0,
         y="dc"),
    dict(name="verify_v2_short", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=15.0,
         y="short"),
    dict(name="verify_v2_silent", seed=301, ch=2, n_fft=4096, hop=2048, x="silent", gain=15.0),
    dict(name="verify_v2_delay100", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=15.0,
         args=dict(up_delay_ms=100.0, hyst_db=3.0)),
    dict(name="verify_v2_loud", seed=301, ch=2, n_fft=4096, hop=2048, x="loud", gain=15.0),
]
L1_CASES = [
    dict(name="verify_l1_st_4096", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=5.0),
    dict(name="verify_l1_mono_2048", seed=302, ch=1, n_fft=2048, hop=512, x="env", gain=5.0),
    dict(name="verify_l1_st_3000", seed=303, ch=2, n_fft=3000, hop=750, x="env", gain=5.0),
    # a +-3 dB output judged against the +-5 dB curves
    dict(name="verify_l1_3db", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=3.0),
    # the state column three rows late
    dict(name="verify_l1_delayed", seed=301, ch=2, n_fft=4096, hop=2048, x="env", gain=5.0,
         csv_delay=3),
]
BY_NAME = {c["name"]: c for c in V2_CASES + L1_CASES}


def make_x(c):
    from tomatis_audio_processor_amd.synth import synth_stream
    if c["x"] == "silent":
        return np.zeros((N, c["ch"]), np.float32)
    x = synth_stream(c["seed"], N, c["ch"], SR).reshape(N, c["ch"])
    if c["x"] == "loud":
        return x
    ph = np.arange(N) % (3 * SR)
    g = np.where((ph >= SR // 100) & (ph < (3 * SR) // 2), np.float32(10.0 ** (10 / 20)),
                 np.float32(10.0 ** (-10 / 20))).astype(np.float32)
    return (x * g[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _base(kind, seed, ch, n_fft, hop, gain):
    """(x, the oracle's result) shared by the cases that differ only afterwards."""
    from oracle import tomatis_oracle as orc
    x = make_x(dict(x=kind, seed=seed, ch=ch))
    ref = orc.process_standard(x, SR, gate_ui=50, gate_mode="linear", gate_scale=1.0,
                               gate_offset=GATE_OFFSET, hysteresis_db=HYST, c1_low=gain,
                               c1_high=-gain, c2_low=-gain, c2_high=gain, up_delay_ms=0.0,
                               n_fft=n_fft, hop=hop)
    y = np.ascontiguousarray(ref["y"], np.float32).reshape(N, ch)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, ref


@functools.lru_cache(maxsize=None)
def _pair(name):
    c = BY_NAME[name]
    x, y, ref = _base(c["x"], c["seed"], c["ch"], c["n_fft"], c["hop"], c["gain"])
    if c.get("y") == "dc":
        y = (y + np.float32(0.002)).astype(np.float32)
    elif c.get("y") == "short":
        y = y[:-1].copy()
    y.setflags(write=False)
    # the rows process_tomatis --state_csv writes: frames that start inside x
    rows = np.nonzero((ref["starts"] >= 0) & (ref["starts"] < N))[0]
    states = np.asarray(ref["states"])[rows].astype(np.int8)
    d = int(c.get("csv_delay", 0))
    if d:
        states = np.concatenate([np.full(d, states[0], np.int8), states[:-d]])
    csv_rows = dict(frame_idx=rows, time_sec=ref["starts"][rows] / SR,
                    level_dbfs=np.asarray(ref["levels"], np.float64)[rows], state=states)
    return x, y, csv_rows


def make_pair(c):
    """-> (x, y, the state-CSV rows as arrays); computed once per case, read-only."""
    return _pair(c["name"])


def write_state_csv(path, rows):
    """The file ``process_tomatis --state_csv`` writes (floats with repr)."""
    import csv
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(["frame_idx", "time_sec", "level_dbfs", "state"])
        for k, t, lv, s in zip(rows["frame_idx"].tolist(), rows["time_sec"].tolist(),
                               rows["level_dbfs"].tolist(), rows["state"].tolist()):
            w.writerow([k, t, lv, "C1" if s == 1 else "C2"])


def csv_frames(rows):
    """The same rows as ``load_state_csv`` returns them."""
    return [dict(frame_idx=int(k), time_sec=float(t), level_dbfs=float(lv),
                 state="C1" if s == 1 else "C2")
            for k, t, lv, s in zip(rows["frame_idx"].tolist(), rows["time_sec"].tolist(),
                                   rows["level_dbfs"].tolist(), rows["state"].tolist())]


def v2_args(c):
    a = dict(V2_DEFAULTS, n_fft=c["n_fft"], hop=c["hop"])
    a.update(c.get("args", {}))
    return a


def l1_args(c):
    a = dict(L1_DEFAULTS, n_fft=c["n_fft"], hop=c["hop"], gate_offset=GATE_OFFSET,
             hyst_db=HYST)
    a.update(c.get("args", {}))
    return a
