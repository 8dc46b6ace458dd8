"""Delay between a recording and a rendered file, on the device (SURVEY.md §8
row f6): ``find_delay_by_corr`` of the reference's workflow scripts
(src/layer2_analyze_eq.py:17-52, src/calibrate_to_baseline_v2.py:46-82).

  reference (layer2_analyze_eq.py)               here
  ---------------------------------------------- ------------------------------
  power_mono :9-11, resample_poly(m, ds_sr, sr),  tomatis_align_envelope (one pass
  ``-= np.mean`` :31-33 / :43-45                  over the PCM, polyphase FIR in LDS)
  fftconvolve(mt_ds, mb_ds[::-1], "valid") :47    tomatis_align_xcorr (direct FMA)
  np.argmax :48                                   tomatis_align_argmax
  chunk bounds :23-27, centres and rounding       host (scalars)
  :49-52

There is one decimating kernel, the polyphase form of resample_poly with the
taps staged by phase, and ``envelope_ds`` and ``envelope_rs`` are two range
checks in front of one body that calls tomatis_align_envelope_rational (the
library's tomatis_align_envelope[_mean_first] are that call with two channels
and up = 1).  ``envelope_ds`` takes ``sr % ds_sr == 0`` with a decimation of
2..64 (48 and 96 kHz; ``device_ratio``), ``envelope_rs`` every ratio up / down
with up < down <= 512 and up <= 64 after reduction (``rational_ratio``:
44.1 kHz is 20 / 441, 88.2 kHz 10 / 441, 176.4 kHz 5 / 441, 192 kHz 1 / 96).
What is left runs the reference's scipy calls on the host
(``_find_delay_host``): up > down, a larger ratio, and a target whose envelope
is shorter than the base chunk's (scipy's ``fftconvolve`` swaps its operands
there).  So does a ratio of ``rational_ratio`` alone on a machine without a
ROCm device; a ratio of ``device_ratio`` has no CPU fallback and raises there.
Inputs are numpy arrays, resident cuda tensors or file paths.

compare_audio's estimate (src/compare_audio.py:30-42) is
the "full" correlation of the two whole envelopes, the mean removed before the
decimation:

  ``resample_poly(m - m.mean(), ds_sr, sr)`` :33-34  tomatis_align_envelope_mean_first
  fftconvolve(c, b[::-1], "full") :37                tomatis_align_xcorr_full (tm_fftcorr.hip)
  np.argmax :38, the shift :39-42                    tomatis_align_argmax, host scalars

``find_delay_full`` picks the range check in the same way and runs
``_find_delay_full_host`` (the reference's scipy body) for a ratio the kernel
does not take and for nc + nb - 1 above 2^25.  ``delay_full_mono`` is the same
estimate on the reference's own arguments, two 1-D power-mono vectors
(``channels == 1`` of the rational entry point, which also takes up = 1).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from . import audio_io
from ._lib import ALIGN_MEAN_DOUBLES, FFT_MAX_LOG2, FFT_MIN_LOG2, check, lib, ptr, stream_handle

EPS = 1e-12
MAX_DOWN = 64  # tm_align.hip kMaxDown
MAX_FULL = 1 << FFT_MAX_LOG2  # lags of xcorr_full (tm_fftcorr.hip kMaxLog)
MAX_DOWN_RS, MAX_UP_RS = 512, 64  # tm_align.hip kRatMaxDown, kRatMaxUp


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("alignment needs a ROCm GPU (MI355X); there is no CPU fallback")
    return torch


def _ratio(sr: int, ds_sr: int):
    g = math.gcd(int(ds_sr), int(sr))
    return int(ds_sr) // g, int(sr) // g  # up, down as resample_poly reduces them


def device_ratio(sr: int, ds_sr: int) -> bool:
    up, down = _ratio(sr, ds_sr)
    return up == 1 and 2 <= down <= MAX_DOWN


def rational_ratio(sr: int, ds_sr: int) -> bool:
    """The ratios tomatis_align_envelope_rational takes (up = 1 included)."""
    up, down = _ratio(sr, ds_sr)
    return 1 <= up < down <= MAX_DOWN_RS and up <= MAX_UP_RS


def _has_device() -> bool:
    try:
        import torch
    except ImportError:
        return False
    return torch.cuda.is_available()


def _n_ds(n: int, up: int, down: int) -> int:
    """len(resample_poly(e, up, down)) for len(e) = n."""
    return -(-n * up // down)


@functools.lru_cache(maxsize=8)
def _taps_rational(up: int, down: int) -> np.ndarray:
    """resample_poly's own filter for float32 input and up < down: the window
    design rounded to float32, then scaled by up in float32."""
    from scipy.signal import firwin
    h = firwin(20 * down + 1, 1.0 / down, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return h


def _taps(down: int) -> np.ndarray:
    """resample_poly's own filter for up = 1 and float32 input."""
    return _taps_rational(1, down)


def _load(a, sr, mono_ok=False):
    """-> (array or cuda tensor [n, 2], or 1-D where ``mono_ok``; is_tensor); the
    reference's asserts."""
    if isinstance(a, str):
        a, got = audio_io.read(a)
        assert got == sr
    is_tensor = not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")
    if not is_tensor:
        a = np.asarray(a)
    assert (mono_ok and a.ndim == 1) or (a.ndim == 2 and a.shape[1] == 2)
    return a, is_tensor


def _stereo_dev(a):
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _vec_dev(a):
    return _stereo_dev(a).reshape(-1)


def _envelope(who, x, sr, ds_sr, start, stop, with_mean, mean_first, mono_ok):
    """The body of ``envelope_ds`` and ``envelope_rs`` once the ratio is checked:
    upload, allocate, one call of tomatis_align_envelope_rational."""
    torch = _torch()
    up, down = _ratio(sr, ds_sr)
    x, is_tensor = _load(x, sr, mono_ok)
    n, ch = x.shape[0], x.ndim
    stop = n if stop is None else min(int(stop), n)
    start = int(start)
    if not 0 <= start < stop:
        raise ValueError(f"{who} needs a non-empty range inside the signal")
    ln = stop - start
    if not is_tensor:  # a host array: only the range is uploaded
        x, n, start = x[start:stop], ln, 0
    xd = _stereo_dev(x)
    taps = torch.from_numpy(_taps_rational(up, down)).cuda()
    out = torch.empty(_n_ds(ln, up, down), dtype=torch.float32, device="cuda")
    mean = torch.empty(ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
    check(lib().tomatis_align_envelope_rational(ptr(xd), n, start, ln, ch, up, down, ptr(taps),
                                                taps.numel(), int(bool(mean_first)), ptr(out),
                                                ptr(mean), stream_handle()),
          "align_envelope_rational")
    return (out, float(mean[0].item())) if with_mean else out


def envelope_ds(x_lr, sr=48000, ds_sr=2000, start=0, stop=None, with_mean=False,
                mean_first=False):
    """``m = resample_poly(power_mono(x_lr[start:stop]), ds_sr, sr).astype(float32);
    m -= np.mean(m)`` as a cuda tensor (``with_mean``: and the mean removed).
    ``mean_first``: compare_audio's order (:33-34), ``m = power_mono(...);
    resample_poly(m - m.mean(), ds_sr, sr)``."""
    _torch()
    if not device_ratio(sr, ds_sr):
        raise ValueError(f"sr={sr}, ds_sr={ds_sr}: the device decimator takes sr % ds_sr == 0 "
                         f"and a factor of 2..{MAX_DOWN}")
    return _envelope("envelope_ds", x_lr, sr, ds_sr, start, stop, with_mean, mean_first, False)


def envelope_rs(x, sr=44100, ds_sr=2000, start=0, stop=None, with_mean=False, mean_first=False):
    """``envelope_ds`` for the ratios of ``rational_ratio``: ``resample_poly(e[start:stop],
    ds_sr, sr)`` with the mean removed after (``mean_first``: before) the
    decimation, as a cuda tensor.  ``x`` is stereo ``[n, 2]`` (e = power_mono) or
    a 1-D vector taken as e itself, in float32."""
    _torch()
    if not rational_ratio(sr, ds_sr):
        raise ValueError(f"sr={sr}, ds_sr={ds_sr}: the rational decimator takes up < down <= "
                         f"{MAX_DOWN_RS} and up <= {MAX_UP_RS}")
    return _envelope("envelope_rs", x, sr, ds_sr, start, stop, with_mean, mean_first, True)


def xcorr_valid(t, b):
    """``fftconvolve(t, b[::-1], mode="valid")`` for len(t) >= len(b): cuda tensor."""
    torch = _torch()
    td, bd = _vec_dev(t), _vec_dev(b)
    nt, nb = td.numel(), bd.numel()
    if nb < 1 or nt < nb:
        raise ValueError("xcorr_valid needs 1 <= len(b) <= len(t)")
    out = torch.empty(nt - nb + 1, dtype=torch.float32, device="cuda")
    check(lib().tomatis_align_xcorr(ptr(td), nt, ptr(bd), nb, ptr(out), stream_handle()),
          "align_xcorr")
    return out


def fft_pow2(x, inverse=False):
    """``np.fft.fft`` / ``np.fft.ifft`` of a complex64 vector of 2^p points,
    FFT_MIN_LOG2 <= p <= FFT_MAX_LOG2 (tomatis_fft_pow2): complex64 cuda tensor."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        xd = x.to(device="cuda", dtype=torch.complex64).contiguous().reshape(-1)
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)).cuda()
    n = xd.numel()
    p = n.bit_length() - 1
    if n < 1 or (1 << p) != n or not FFT_MIN_LOG2 <= p <= FFT_MAX_LOG2:
        raise ValueError(f"fft_pow2 takes 2^{FFT_MIN_LOG2} .. 2^{FFT_MAX_LOG2} points, not {n}")
    work = torch.empty(int(lib().tomatis_fft_pow2_work_bytes(p)), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(xd)
    check(lib().tomatis_fft_pow2(ptr(xd), ptr(out), p, int(bool(inverse)), ptr(work),
                                 stream_handle()), "fft_pow2")
    return out


def xcorr_full(c, b):
    """``fftconvolve(c, b[::-1], mode="full")`` (compare_audio.py:37): cuda tensor
    of len(c) + len(b) - 1 lags, out[k] = sum_j c[k - (len(b) - 1) + j] b[j]."""
    torch = _torch()
    cd, bd = _vec_dev(c), _vec_dev(b)
    nc, nb = cd.numel(), bd.numel()
    if nc < 1 or nb < 1:
        raise ValueError("xcorr_full needs non-empty inputs")
    if nc + nb - 1 > MAX_FULL:
        raise ValueError(f"xcorr_full takes len(c) + len(b) - 1 <= {MAX_FULL}")
    work = torch.empty(int(lib().tomatis_align_xcorr_full_work_bytes(nc, nb)), dtype=torch.uint8,
                       device="cuda")
    out = torch.empty(nc + nb - 1, dtype=torch.float32, device="cuda")
    check(lib().tomatis_align_xcorr_full(ptr(cd), nc, ptr(bd), nb, ptr(out), ptr(work),
                                         stream_handle()), "align_xcorr_full")
    return out


def argmax_first(c, with_value=False):
    """``int(np.argmax(c))``: the lowest index of the maximum."""
    torch = _torch()
    cd = _vec_dev(c)
    idx = torch.empty(1, dtype=torch.int64, device="cuda")
    val = torch.empty(1, dtype=torch.float32, device="cuda")
    check(lib().tomatis_align_argmax(ptr(cd), cd.numel(), ptr(idx), ptr(val), stream_handle()),
          "align_argmax")
    k = int(idx.item())
    return (k, float(val.item())) if with_value else k


def _chunk(nbase: int, sr: int, chunk_sec):
    """The middle chunk_sec of the base, clamped to the file (:23-27)."""
    mid = int(0.5 * nbase)
    half = int(0.5 * chunk_sec * sr)
    return max(0, mid - half), min(nbase, mid + half)


def _delay(k: int, n_ds: int, s: int, e: int, sr: int, ds_sr: int) -> int:
    """:49-52."""
    base_center_sec = (s + (e - s) // 2) / sr
    targ_center_sec = (k + n_ds // 2) / ds_sr
    delay_sec = targ_center_sec - base_center_sec
    return int(round(delay_sec * sr))


def power_mono(x_lr: np.ndarray) -> np.ndarray:
    """layer2_analyze_eq.py:9-11 (host)."""
    p = 0.5 * (x_lr[:, 0] * x_lr[:, 0] + x_lr[:, 1] * x_lr[:, 1])
    return np.sqrt(p + EPS)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _find_delay_host(target, base, sr=48000, ds_sr=2000, chunk_sec=25):
    """The reference's own scipy calls on the host (:17-52), for the cases the
    device path leaves out."""
    from scipy.signal import fftconvolve, resample_poly
    xt, _ = _load(target, sr)
    xb, _ = _load(base, sr)
    xt, xb = _host(xt).astype(np.float32, copy=False), _host(xb).astype(np.float32, copy=False)
    s, e = _chunk(len(xb), sr, chunk_sec)
    mb = power_mono(xb[s:e])
    mb_ds = resample_poly(mb, ds_sr, sr).astype(np.float32)
    mb_ds = mb_ds - np.mean(mb_ds)
    mt = power_mono(xt).astype(np.float32)
    mt_ds = resample_poly(mt, ds_sr, sr).astype(np.float32)
    mt_ds = mt_ds - np.mean(mt_ds)
    corr = fftconvolve(mt_ds, mb_ds[::-1], mode="valid")
    k = int(np.argmax(corr))
    return _delay(k, len(mb_ds), s, e, sr, ds_sr)


def _decimator(sr, ds_sr):
    """``envelope_ds`` where it applies, else ``envelope_rs``, else None (the host)."""
    if device_ratio(sr, ds_sr):
        return envelope_ds
    if rational_ratio(sr, ds_sr) and _has_device():
        return envelope_rs
    return None


def find_delay(target, base, sr=48000, ds_sr=2000, chunk_sec=25):
    """delay = target - base in samples (positive: the target starts later),
    layer2_analyze_eq.find_delay_by_corr (:17-52)."""
    xt, _ = _load(target, sr)
    xb, _ = _load(base, sr)
    s, e = _chunk(len(xb), sr, chunk_sec)
    env = _decimator(sr, ds_sr)
    if env is None:
        return _find_delay_host(xt, xb, sr, ds_sr, chunk_sec)
    up, down = _ratio(sr, ds_sr)
    if e <= s or len(xt) < 1 or _n_ds(len(xt), up, down) < _n_ds(e - s, up, down):
        return _find_delay_host(xt, xb, sr, ds_sr, chunk_sec)
    mb_ds = env(xb, sr, ds_sr, s, e)
    mt_ds = env(xt, sr, ds_sr)
    k = argmax_first(xcorr_valid(mt_ds, mb_ds))
    return _delay(k, mb_ds.numel(), s, e, sr, ds_sr)


def _delay_full(k: int, nb: int, sr: int, ds_sr: int) -> int:
    """compare_audio.py:39-41."""
    shift_ds = k - (nb - 1)
    return int(round(shift_ds * (sr / ds_sr)))


def _delay_full_host(base_mono, cand_mono, sr, ds_sr=2000):
    """The reference's own scipy calls on the host (compare_audio.py:30-42) on
    the two power-mono signals."""
    from scipy.signal import fftconvolve, resample_poly
    b = resample_poly(base_mono - base_mono.mean(), ds_sr, sr).astype(np.float32)
    c = resample_poly(cand_mono - cand_mono.mean(), ds_sr, sr).astype(np.float32)
    corr = fftconvolve(c, b[::-1], mode="full")
    return _delay_full(int(np.argmax(corr)), len(b), sr, ds_sr)


def _find_delay_full_host(base, cand, sr=48000, ds_sr=2000):
    """``_delay_full_host`` of two stereo signals, for the cases the device path
    leaves out."""
    xb, _ = _load(base, sr)
    xc, _ = _load(cand, sr)
    return _delay_full_host(power_mono(_host(xb).astype(np.float32, copy=False)),
                            power_mono(_host(xc).astype(np.float32, copy=False)), sr, ds_sr)


def find_delay_full(base, cand, sr=48000, ds_sr=2000):
    """delay = cand - base in samples from the full correlation of the whole
    envelopes, compare_audio.find_delay_by_corr (:30-42)."""
    xb, _ = _load(base, sr)
    xc, _ = _load(cand, sr)
    env = _decimator(sr, ds_sr)
    if env is None or len(xb) < 1 or len(xc) < 1:
        return _find_delay_full_host(xb, xc, sr, ds_sr)
    up, down = _ratio(sr, ds_sr)
    if _n_ds(len(xb), up, down) + _n_ds(len(xc), up, down) - 1 > MAX_FULL:
        return _find_delay_full_host(xb, xc, sr, ds_sr)
    b = env(xb, sr, ds_sr, mean_first=True)
    c = env(xc, sr, ds_sr, mean_first=True)
    k = argmax_first(xcorr_full(c, b))
    return _delay_full(k, b.numel(), sr, ds_sr)


def delay_full_mono(base_mono, cand_mono, sr, ds_sr=2000):
    """``find_delay_full`` on the reference's own arguments, two 1-D power-mono
    vectors (arrays or resident tensors), taken as float32.  The host body for a
    ratio the rational decimator does not take and above 2^25 lags."""
    up, down = _ratio(sr, ds_sr)
    nb, nc = len(base_mono), len(cand_mono)
    if (not (rational_ratio(sr, ds_sr) and _has_device()) or nb < 1 or nc < 1
            or _n_ds(nb, up, down) + _n_ds(nc, up, down) - 1 > MAX_FULL):
        return _delay_full_host(_host(base_mono), _host(cand_mono), sr, ds_sr)
    b = envelope_rs(base_mono, sr, ds_sr, mean_first=True)
    c = envelope_rs(cand_mono, sr, ds_sr, mean_first=True)
    k = argmax_first(xcorr_full(c, b))
    return _delay_full(k, b.numel(), sr, ds_sr)


__all__ = ["envelope_ds", "envelope_rs", "xcorr_valid", "fft_pow2", "xcorr_full", "argmax_first",
           "find_delay", "find_delay_full", "delay_full_mono", "device_ratio", "rational_ratio",
           "power_mono"]
