"""Analysis spectra on the device: the validators' and calibration tools' STFTs
(SURVEY.md §8 rows f3/f4), same names, arguments, return values and errors as
the reference functions:

  stft_mag_avg                  src/compare_audio.py:12-24
  power_mono                    src/compare_audio.py:7-10
  stft_logpower_median          src/layer2_analyze_eq.py:54-88
  find_stable_frames            src/validate_layer1.py:245-258 (host: list logic)
  compute_conditional_spectrum  src/validate_layer1.py:261-389

and, below them, the device pieces the two acceptance validators share
(validate_layer1.py, verify_tomatis_15db_v2.py; row f9): the padded level grid,
the gate scan, the anchored ratio rows and band energies, peak and float64 sum;
and the two the parameter-recovery tools share (reverse_engineer_params.py,
verify_tilt_amplitude.py; row f11): ``pair_tilt`` and ``pair_diff_mean``.

Everything per frame or per sample runs in ``libtomatis_hip.so``
(``tm_analysis.hip``): framing, power-mono premix, window, real FFT (two real
frames per complex FFT), |X| / log-power / Y-over-X ratios, the per-frame
level (bit-exact numpy pairwise order) and its gate predicate, the mean and the
median over frames.  The host keeps once-per-call set-up (window, rfftfreq,
the level threshold as r bit patterns via ``dsp.gate_bits``, the stable-frame
classes from the state list) and the bins-sized final ``20*log10`` of the
validator.  Inputs may be numpy arrays (uploaded) or resident cuda tensors.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import dsp
from ._lib import check, lib, ptr, stream_handle

EPS = 1e-12
AN_LEVEL_CHMEAN, AN_LEVEL_POWER_MONO = 0, 1
AN_SIG_RAW, AN_SIG_POWER_MONO = 0, 1
AN_MAG, AN_LOGPOW, AN_RATIO = 0, 1, 2
MIN_N_FFT = 16               # tm_analysis.hip kMinN
MAX_N_FFT = 16384            # kMaxM: one FFT in LDS
MAX_N_FFT_BLUESTEIN = 8192   # 2 n_fft - 1 <= kMaxM


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("analysis spectra need a ROCm GPU (MI355X); there is no CPU fallback")
    return torch


def _dev(a, ch=None):
    """float32 contiguous cuda tensor of shape [n] or [n, ch]."""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        t = a.to(device="cuda", dtype=torch.float32).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()
    if ch is not None and t.dim() == 1:
        t = t.reshape(-1, 1)
    return t


def _check_n_fft(n_fft):
    """Any length np.fft.rfft takes, within the LDS: powers of two in
    [16, MAX_N_FFT], other lengths in [16, MAX_N_FFT_BLUESTEIN] (Bluestein's
    chirp-z runs a power-of-two FFT of >= 2 n_fft - 1 points)."""
    pow2 = n_fft > 0 and (n_fft & (n_fft - 1)) == 0
    cap = MAX_N_FFT if pow2 else MAX_N_FFT_BLUESTEIN
    if n_fft < MIN_N_FFT or n_fft > cap:
        raise ValueError(f"n_fft={n_fft}: the analysis kernels take {MIN_N_FFT} <= n_fft <= "
                         f"{cap} ({'power of two' if pow2 else 'Bluestein'}), as tm_analysis.hip")


def _n_frames(n, n_fft, hop):
    return 1 + (n - n_fft) // hop  # Python floor division, as the reference loops


def _spectra(x, y, n, ch, n_fft, hop, kind, sig, scale=1.0):
    torch = _torch()
    F = _n_frames(n, n_fft, hop)
    nb = n_fft // 2 + 1
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    out = torch.empty((F, nb), dtype=torch.float32, device="cuda")
    check(lib().tomatis_an_spectra(ptr(x), ptr(y), n, ch, n_fft, hop, kind, sig,
                                   C.c_float(scale), ptr(win), ptr(out), stream_handle()),
          "an_spectra")
    return out


def _frame_r(x, n, ch, n_fft, hop, mode, scale=1.0):
    torch = _torch()
    r = torch.empty(_n_frames(n, n_fft, hop), dtype=torch.float32, device="cuda")
    check(lib().tomatis_an_frame_r(ptr(x), n, ch, n_fft, hop, mode, C.c_float(scale), ptr(r),
                                   stream_handle()), "an_frame_r")
    return r


def _select(r, thr_bits, exc, keep_above, cls=None, cls_want=0):
    """Device frame mask from exact level predicates; returns (mask, count)."""
    torch = _torch()
    F = r.numel()
    mask = torch.empty(F, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    ex = (C.c_uint32 * 4)(*(list(exc) + [0] * (4 - len(exc))))
    check(lib().tomatis_an_select(ptr(r), F, thr_bits, ex, len(exc), keep_above, ptr(cls),
                                  cls_want, ptr(mask), ptr(cnt), stream_handle()), "an_select")
    return mask, int(cnt.item())


def frame_median(spec, mask=None, n_sel=None):
    """np.median(spec[mask], axis=0) on the device (float32, numpy's even rule)."""
    torch = _torch()
    F, nb = spec.shape
    n_sel = F if n_sel is None else n_sel
    work = torch.empty(int(lib().tomatis_an_median_work_words(nb)), dtype=torch.int32,
                       device="cuda")
    out = torch.empty(nb, dtype=torch.float32, device="cuda")
    check(lib().tomatis_an_frame_median(ptr(spec), F, nb, ptr(mask), n_sel, ptr(work), ptr(out),
                                        stream_handle()), "an_frame_median")
    return out


def frame_mean(spec):
    """spec.mean(axis=0) on the device in numpy's axis-0 order."""
    torch = _torch()
    F, nb = spec.shape
    out = torch.empty(nb, dtype=torch.float32, device="cuda")
    check(lib().tomatis_an_frame_mean(ptr(spec), F, nb, ptr(out), stream_handle()),
          "an_frame_mean")
    return out


# ---------------------------------------------------------------------------
# reference-named functions
# ---------------------------------------------------------------------------

def power_mono(x_lr):
    """compare_audio.py:7-10 — host numpy (elementwise, used for inputs/CSV only).
    The device fuses the same formula into the spectrum and level kernels."""
    p = 0.5 * (x_lr[:, 0] ** 2 + x_lr[:, 1] ** 2)
    return np.sqrt(p + EPS)


def stft_mag_avg(x, sr, n_fft=4096, hop=2048, *, premix=None, scale=1.0, as_tensor=False):
    """compare_audio.stft_mag_avg: mean over frames of |rfft(win * x[f*hop:+n_fft])|.

    ``x`` is the mono signal (1-D), or with ``premix="power_mono"`` the stereo
    ``[n, 2]`` whose power mono the reference would pass (fused on the device).
    ``scale`` multiplies the PCM first (compare_audio.py:82-86 scales the
    candidate before power_mono)."""
    _check_n_fft(n_fft)
    if premix == "power_mono":
        xd = _dev(x, ch=2)
        if xd.shape[1] != 2:
            raise ValueError("power_mono premix needs a stereo [n, 2] input")
        sig, ch = AN_SIG_POWER_MONO, 2
    else:
        xd = _dev(x).reshape(-1)
        sig, ch = AN_SIG_RAW, 1
    n = xd.shape[0]
    if _n_frames(n, n_fft, hop) <= 0:
        raise ValueError("need at least one array to stack")  # np.stack([]) in the reference
    spec = _spectra(xd, None, n, ch, n_fft, hop, AN_MAG, sig, scale)
    m = frame_mean(spec)
    return m if as_tensor else m.cpu().numpy()


def stft_logpower_median(x_lr, sr: int, n_fft: int, hop: int, music_dbfs: float):
    """layer2_analyze_eq.stft_logpower_median -> (freqs, median_logP_dB, used_frames).

    Frames whose power-mono level is <= music_dbfs are dropped (exact, on the bit
    pattern of r); the median over the kept frames of 10 log10(|X|^2 + EPS)."""
    _check_n_fft(n_fft)
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    xd = _dev(x_lr, ch=2)
    if xd.shape[1] != 2:
        raise ValueError("stft_logpower_median expects a stereo [n, 2] input")
    n = xd.shape[0]
    F = _n_frames(n, n_fft, hop)
    if F <= 10:
        raise ValueError("片段太短，无法做稳定频谱统计。")
    r = _frame_r(xd, n, 2, n_fft, hop, AN_LEVEL_POWER_MONO)
    _, _, off_bits, off_exc = dsp.gate_bits(float(music_dbfs), float(music_dbfs))
    mask, used = _select(r, off_bits, off_exc, keep_above=0)
    if used < 50:
        raise ValueError(f"可用音乐帧太少（{used} 帧）。把 --music_dbfs 调低一点（例如 -70）。")
    spec = _spectra(xd, None, n, 2, n_fft, hop, AN_LOGPOW, AN_SIG_POWER_MONO)
    med = frame_median(spec, mask, used)
    return freqs, med.cpu().numpy(), used


def stable_classes(codes, margin=2):
    """find_stable_frames' rule on int8 codes: 1 / 2 where the +-margin window is
    all C1 / all C2, else 0."""
    codes = np.asarray(codes, np.int8)
    n = len(codes)
    cls = np.zeros(n, np.int8)
    if n - 2 * margin <= 0:
        return cls
    win = np.lib.stride_tricks.sliding_window_view(codes, 2 * margin + 1)
    cls[margin:n - margin][np.all(win == 1, axis=1)] = 1
    cls[margin:n - margin][np.all(win == 2, axis=1)] = 2
    return cls


def _stable_classes(states, margin=2):
    """int8 per state index: 1 = stable C1, 2 = stable C2, 0 = neither
    (validate_layer1.find_stable_frames' rule, vectorised)."""
    s = None
    try:  # fast path: a list of "C1"/"C2" strings joined into one byte buffer
        b = np.frombuffer("".join(states).encode("ascii"), np.uint8)
        if b.size == 2 * len(states) and np.all(b[0::2] == ord("C")):
            d = b[1::2]
            s = np.where(d == ord("1"), 1, np.where(d == ord("2"), 2, 0)).astype(np.int8)
    except (TypeError, UnicodeEncodeError):
        s = None
    if s is None:
        s = np.asarray([1 if v == "C1" else (2 if v == "C2" else 0) for v in states], np.int8)
    return stable_classes(s, margin)


def find_stable_frames(states, margin=2):
    """validate_layer1.find_stable_frames: indices whose +-margin window is all
    C1 (first list) or all C2 (second list)."""
    cls = _stable_classes(states, margin)
    return np.nonzero(cls == 1)[0].tolist(), np.nonzero(cls == 2)[0].tolist()


def compute_conditional_spectrum(x, y, sr, states, n_fft, hop, level_threshold=-60):
    """validate_layer1.compute_conditional_spectrum ->
    (freqs, c1_db, c2_db, n_c1_frames, n_c2_frames).

    Per stable frame (fully inside x, level >= level_threshold) the ratio
    mean_c|Y_c| / max(mean_c|X_c|, 1e-10); median over frames per class;
    20 log10(median + EPS)."""
    _check_n_fft(n_fft)
    torch = _torch()
    xd = _dev(x, ch=True)
    yd = _dev(y, ch=True)
    n, ch = xd.shape
    if ch not in (1, 2) or yd.shape[1] != ch:
        raise ValueError("x and y must have the same channel count (1 or 2)")
    if yd.shape[0] < n:
        raise ValueError("y must be at least as long as x")
    yd = yd[:n].contiguous()
    freqs = np.fft.rfftfreq(n_fft, 1 / sr)
    nb = len(freqs)
    F = max(0, _n_frames(n, n_fft, hop))  # frames idx with idx*hop + n_fft <= len(x)
    cls = np.zeros(F, np.int8)
    sc = _stable_classes(states, margin=2)[:F]
    cls[:len(sc)] = sc
    out = []
    if F > 0:
        r = _frame_r(xd, n, ch, n_fft, hop, AN_LEVEL_CHMEAN)
        on_bits, on_exc, _, _ = dsp.gate_bits(float(level_threshold), float(level_threshold))
        cls_d = torch.from_numpy(cls).cuda()
        sel = [_select(r, on_bits, on_exc, keep_above=1, cls=cls_d, cls_want=v) for v in (1, 2)]
        spec = _spectra(xd, yd, n, ch, n_fft, hop, AN_RATIO, AN_SIG_RAW) \
            if any(c for _, c in sel) else None
    else:
        sel = [(None, 0), (None, 0)]
    for mask, cnt in sel:
        if cnt:
            med = frame_median(spec, mask, cnt).cpu().numpy()
            out.append(20 * np.log10(med + EPS))
        else:
            out.append(np.zeros(nb))
    return freqs, out[0], out[1], sel[0][1], sel[1][1]


# ---------------------------------------------------------------------------
# acceptance validators: the device pieces shared by
# validate_layer1.py and verify_tomatis_15db_v2.py
# ---------------------------------------------------------------------------

def band_bins(freqs, f_lo, f_hi):
    """[b0, b1): the bins with f_lo <= freqs <= f_hi (both ends included, as the
    validators' masks); (0, 0) when there is none."""
    idx = np.nonzero((freqs >= f_lo) & (freqs <= f_hi))[0]
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def pair_on_device(x, y, max_short):
    """x and y as resident [n, ch] tensors of one length: y is cut to len(x), or
    zero-extended when it is shorter by at most ``max_short`` frames (what the
    validators' n_fft // 2 of zero padding does to a frame that runs past y)."""
    torch = _torch()
    xd = _dev(x, ch=True)
    yd = _dev(y, ch=True)
    n, ch = xd.shape
    if ch not in (1, 2) or yd.shape[1] != ch:
        raise ValueError("x and y must have the same channel count (1 or 2)")
    if yd.shape[0] < n:
        if n - yd.shape[0] > max_short:
            raise ValueError(f"y is {n - yd.shape[0]} frames shorter than x (at most {max_short})")
        yd = torch.cat([yd, torch.zeros((n - yd.shape[0], ch), dtype=torch.float32,
                                        device="cuda")])
    return xd, yd[:n].contiguous()


def padded_frame_levels(xd, n_fft, hop):
    """The validators' level grid (validate_layer1.py:116-161,
    verify_tomatis_15db_v2.py:107-123): x zero-padded by n_fft // 2 on both sides
    on the device, frames at k * hop of the padded signal while they fit, kept
    where 0 <= k * hop - n_fft // 2 < n  ->  (levels float64, padded starts int64).
    r comes from tomatis_an_frame_r (bit-exact); the level is the reference's own
    numpy expression on the host (dsp.r_to_level)."""
    torch = _torch()
    n, ch = xd.shape
    pad = n_fft // 2
    if n == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    xp = torch.zeros((n + 2 * pad, ch), dtype=torch.float32, device="cuda")
    xp[pad:pad + n] = xd
    r = _frame_r(xp, n + 2 * pad, ch, n_fft, hop, AN_LEVEL_CHMEAN).cpu().numpy()
    s = np.arange(len(r), dtype=np.int64) * hop
    keep = (s - pad >= 0) & (s - pad < n)
    return dsp.r_to_level(r[keep]), s[keep]


def state_codes(states):
    """int8 1 / 2 per state from a list of 'C1' / 'C2' (or an integer array)."""
    if isinstance(states, np.ndarray) and states.dtype.kind in "iu":
        return states.astype(np.int8)
    if len(states) == 0:
        return np.zeros(0, np.int8)
    b = np.frombuffer("".join(states).encode("ascii"), np.uint8)
    if b.size != 2 * len(states):
        raise ValueError("states must be 'C1' / 'C2'")
    return np.where(b[1::2] == ord("2"), 2, 1).astype(np.int8)


def state_names(codes):
    return np.where(np.asarray(codes) == 2, "C2", "C1").tolist()


def _f32_at_least(v):
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


def _f32_at_most(v):
    f = np.float32(v)
    return f if float(f) <= v else np.nextafter(f, np.float32(-np.inf))


class GateScan:
    """The validators' gate automaton (validate_layer1.py:141-157,
    verify_tomatis_15db_v2.py:126-152) over resident levels: one
    tomatis_cal_gate_grid launch per threshold pair.  The levels are float32
    values held in float64, which the reference compares with float64 thresholds;
    the kernel gets the smallest float32 >= Ton and the largest <= Toff, so every
    comparison comes out as the reference's."""

    def __init__(self, levels, starts):
        torch = _torch()
        lv64 = np.asarray(levels, np.float64)
        lv32 = lv64.astype(np.float32)
        if not np.array_equal(lv32.astype(np.float64), lv64, equal_nan=True):
            raise ValueError("gate levels must be float32 values (20 log10(r + EPS) of a float32 r)")
        self.n = len(lv32)
        self.lv = torch.from_numpy(lv32).cuda()
        self.st = torch.from_numpy(np.ascontiguousarray(starts, np.int64)).cuda()
        self.tg = torch.ones(max(1, self.n), dtype=torch.int32, device="cuda")  # all C1
        self.out = torch.empty(2, dtype=torch.int32, device="cuda")
        self.states = None

    def run(self, Ton, Toff, up_delay, want_states=False):
        """-> (C2 count, switch count[, int8 states])."""
        from ._lib import GATE_CAND_DTYPE
        torch = _torch()
        if self.n == 0:
            return (0, 0, np.zeros(0, np.int8)) if want_states else (0, 0)
        c = np.zeros(1, GATE_CAND_DTYPE)
        c["t_on"], c["t_off"] = _f32_at_least(float(Ton)), _f32_at_most(float(Toff))
        c["up_delay"] = int(up_delay)
        cb = torch.from_numpy(c.view(np.uint8)).cuda()
        if want_states and self.states is None:
            self.states = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        check(lib().tomatis_cal_gate_grid(ptr(self.lv), self.n, ptr(self.st), ptr(self.tg),
                                          ptr(cb), 1, ptr(self.out),
                                          ptr(self.states if want_states else None),
                                          stream_handle()), "cal_gate_grid")
        c2, sw = (int(v) for v in self.out.cpu().numpy())
        if want_states:
            return c2, sw, self.states.cpu().numpy().astype(np.int8)
        return c2, sw


def verify_spectra(xd, yd, n_fft, hop, anchor=None, bands=None, fused=True, win=None):
    """The validator's per-frame spectra of a resident pair (tm_analysis.hip
    k_an_verify): the anchored ratio rows [F, n_fft/2+1] for ``anchor`` = (a0, a1)
    and / or the band energies [F, 4] for ``bands`` = (lo0, lo1, hi0, hi1).  With
    both, one launch forms them from one transform (``fused``), or two launches
    do; the bits are the same.  ``win``: the resident float32 Hann window, where the
    caller keeps one (default: built and uploaded here)."""
    _check_n_fft(n_fft)
    torch = _torch()
    n, ch = xd.shape
    F = max(0, _n_frames(n, n_fft, hop))
    nb = n_fft // 2 + 1
    if win is None:
        win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    rows = torch.empty((F, nb), dtype=torch.float32, device="cuda") if anchor is not None else None
    be = torch.empty((F, 4), dtype=torch.float32, device="cuda") if bands is not None else None
    if F == 0:
        return rows, be
    L, hs = lib(), stream_handle()
    if rows is not None and be is not None and fused:
        check(L.tomatis_an_verify_pair(ptr(xd), ptr(yd), n, ch, n_fft, hop, *anchor, *bands,
                                       ptr(win), ptr(rows), ptr(be), hs), "an_verify_pair")
        return rows, be
    if rows is not None:
        check(L.tomatis_an_anchored_ratio(ptr(xd), ptr(yd), n, ch, n_fft, hop, *anchor, ptr(win),
                                          ptr(rows), hs), "an_anchored_ratio")
    if be is not None:
        check(L.tomatis_an_pair_band_energy(ptr(xd), ptr(yd), n, ch, n_fft, hop, *bands, ptr(win),
                                            ptr(be), hs), "an_pair_band_energy")
    return rows, be


# ---------------------------------------------------------------------------
# parameter recovery: the device pieces shared by
# reverse_engineer_params.py and verify_tilt_amplitude.py
# ---------------------------------------------------------------------------

def pair_tilt(xd, yd, n_fft, hop, lo, hi, want_rows=False):
    """Per frame of a resident stereo pair the means of d = 20 log10(|B| + EPS) -
    20 log10(|A| + EPS) (A, B the power-mono spectra of x and y) over the bin
    ranges ``lo`` = (lo0, lo1) and ``hi`` = (hi0, hi1): a float64 tensor [F, 2]
    (tm_analysis.hip k_an_pair_tilt), and with ``want_rows`` the float32 rows
    [F, n_fft/2+1] as well -> (band_means, rows or None)."""
    _check_n_fft(n_fft)
    torch = _torch()
    n, ch = xd.shape
    if ch != 2 or tuple(yd.shape) != (n, 2):
        raise ValueError("x and y must be stereo and of one length")
    F = max(0, _n_frames(n, n_fft, hop))
    nb = n_fft // 2 + 1
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    means = torch.empty((F, 2), dtype=torch.float64, device="cuda")
    rows = torch.empty((F, nb), dtype=torch.float32, device="cuda") if want_rows else None
    check(lib().tomatis_an_pair_tilt(ptr(xd), ptr(yd), n, n_fft, hop, *lo, *hi, ptr(win),
                                     ptr(rows), ptr(means), stream_handle()), "an_pair_tilt")
    return means, rows


def pair_diff_mean(xd, yd, n_fft, hop, frames=None):
    """The float64 mean over ``frames`` (ascending frame indices; default: every
    frame) of the rows d of ``pair_tilt``: a float64 tensor [n_fft/2+1]
    (tm_analysis.hip k_an_pair_diff_mean), NaN for an empty list.  The list stays
    on the host: the library checks it and copies it behind its workspace."""
    _check_n_fft(n_fft)
    torch = _torch()
    n, ch = xd.shape
    if ch != 2 or tuple(yd.shape) != (n, 2):
        raise ValueError("x and y must be stereo and of one length")
    F = max(0, _n_frames(n, n_fft, hop))
    nb = n_fft // 2 + 1
    L = lib()
    if frames is None:
        fl, n_sel = None, F
    else:
        fl = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        n_sel = len(fl)
        if n_sel == 0:
            fl = np.zeros(1, np.int32)   # an empty list, not NULL (= every frame)
    win = torch.from_numpy(dsp.hann(n_fft)).cuda()
    work = torch.empty(max(1, int(L.tomatis_an_pair_diff_mean_work_doubles(n_sel, nb))),
                       dtype=torch.float64, device="cuda")
    out = torch.full((nb,), float("nan"), dtype=torch.float64, device="cuda")
    check(L.tomatis_an_pair_diff_mean(ptr(xd), ptr(yd), n, n_fft, hop, ptr(win),
                                      None if fl is None else fl.ctypes.data_as(C.c_void_p),
                                      n_sel, ptr(work), ptr(out), stream_handle()),
          "an_pair_diff_mean")
    return out


def sum_f64(t):
    """Float64 sum of a resident float32 tensor (tomatis_sum_f64: fixed order)."""
    from ._lib import SUM_DOUBLES
    torch = _torch()
    t = t.reshape(-1)
    out = torch.empty(SUM_DOUBLES, dtype=torch.float64, device="cuda")
    check(lib().tomatis_sum_f64(ptr(t), t.numel(), ptr(out), stream_handle()), "sum_f64")
    return float(out[0].item())


def absmax(t):
    """np.max(np.abs(t)) of a resident float32 tensor as np.float32 (tomatis_absmax)."""
    torch = _torch()
    t = t.reshape(-1)
    bits = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(lib().tomatis_absmax(ptr(t), t.numel(), ptr(bits), stream_handle()), "absmax")
    return np.array([bits.item()], np.int32).view(np.float32)[0]
