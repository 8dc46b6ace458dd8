"""The audio resampler of workflow step 2.1 on the device (SURVEY.md §8 row
f10): ``scipy.signal.resample_poly(x, up, down, axis=0)`` for multichannel PCM,
the call the reference makes wherever it changes a rate, as one polyphase pass
(``tomatis_resample_poly``, csrc/tm_resample.hip).

  reference / workflow                              here
  ------------------------------------------------- ----------------------------
  resample_poly's filter for float32 input           ``taps`` (host, cached)
  resample_poly(x[start:stop], up, down, axis=0)     ``resample_poly``
  ``ffmpeg -ss .. -t .. -ar 48000`` of the workflow  ``resample_to`` (the range is
                                                     the kernel's start / len)

The kernel takes every reduced ratio with max(up, down) <= 512 and
down <= 8 up, and 1..8 channels: 44.1 kHz -> 48 kHz is 160 / 147, 96 kHz 1 / 2,
192 kHz 1 / 4 (``supported``).  A ratio outside raises ``ValueError``: there is
no host fallback.  Inputs are numpy arrays ``[n]`` / ``[n, ch]`` or resident
cuda tensors; a host array uploads only its range.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from ._lib import check, lib, ptr, stream_handle

MAX_RATIO = 512   # csrc/tm_resample_plan.h kMaxRatio: max(up, down)
MAX_DECIM = 8     # kMaxDecim: down <= MAX_DECIM up
MAX_CH = 8        # kMaxCh
MAX_TILE = 1024   # kMaxTile
LDS_BYTES = 64 * 1024


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the resampler needs a ROCm GPU (MI355X); there is no CPU fallback")
    return torch


def ratio(sr: int, target_sr: int):
    """(up, down) as resample_poly reduces them."""
    g = math.gcd(int(sr), int(target_sr))
    return int(target_sr) // g, int(sr) // g


def _in_limits(up: int, down: int) -> bool:
    return up >= 1 and down >= 1 and max(up, down) <= MAX_RATIO and down <= MAX_DECIM * up


def supported(sr: int, target_sr: int) -> bool:
    """Whether ``resample_to(x, sr, target_sr)`` runs (equal rates: a copy)."""
    return _in_limits(*ratio(sr, target_sr))


def _limits_text() -> str:
    return (f"the device resampler takes max(up, down) <= {MAX_RATIO} and down <= {MAX_DECIM} up "
            f"after reduction, and 1..{MAX_CH} channels")


@functools.lru_cache(maxsize=16)
def taps(up: int, down: int) -> np.ndarray:
    """resample_poly's own filter for float32 input: the window design rounded to
    float32, then scaled by up in float32 (do not write to the cached array)."""
    from scipy.signal import firwin
    m = max(int(up), int(down))
    h = firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    h.setflags(write=False)
    return h


def n_out(n: int, up: int, down: int) -> int:
    """len(resample_poly(x, up, down)) for len(x) = n."""
    return -(-int(n) * up // down)


def outputs_per_workgroup(up: int, down: int, channels: int, n_taps=None,
                          lds_bytes: int = LDS_BYTES) -> int:
    """T of csrc/tm_resample_plan.h's rs_plan: the largest power of two <= 1024
    consecutive output frames whose staged samples and phase table fit the LDS
    budget.  ``lds_words`` gives the words it then uses.  A mirror of the C
    code, held to it by tests/test_resample_plan.py."""
    return _plan(up, down, channels, n_taps, lds_bytes)[0]


def lds_words(up: int, down: int, channels: int, n_taps=None) -> int:
    return _plan(up, down, channels, n_taps, LDS_BYTES)[1]


def _plan(up, down, channels, n_taps, lds_bytes):
    n_taps = 20 * max(up, down) + 1 if n_taps is None else int(n_taps)
    K = -(-n_taps // up)
    K4 = -(-K // 4) * 4
    Ks = 4 * (-(-K // 4) | 1)
    tab = up * Ks
    T = MAX_TILE
    while T >= 1:
        W = (up - 1 + down * (T - 1)) // up + K4
        stage = (3 + W * channels + 3) // 4 * 4
        if 4 * (stage + tab) <= lds_bytes:
            return T, stage + tab
        T //= 2
    raise ValueError((up, down, channels, n_taps))


def _upload(a):
    """A host array (or a slice of one) as a float32 cuda tensor."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not a.flags.writeable:  # torch refuses to wrap a read-only array
        a = a.copy()
    return torch.from_numpy(a).cuda()


def _as_device(x):
    """-> (float32 cuda tensor, flat and contiguous; n; ch; rank)."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        if x.ndim not in (1, 2):
            raise ValueError("resample_poly takes [n] or [n, ch]")
        return x.to(device="cuda", dtype=torch.float32).contiguous(), x.shape[0], \
            (1 if x.ndim == 1 else x.shape[1]), x.ndim
    a = np.asarray(x)
    if a.ndim not in (1, 2):
        raise ValueError("resample_poly takes [n] or [n, ch]")
    return a, a.shape[0], (1 if a.ndim == 1 else a.shape[1]), a.ndim


def resample_poly(x, up: int, down: int, start: int = 0, stop=None):
    """``scipy.signal.resample_poly(x[start:stop], up, down, axis=0)`` with its
    default filter, as a float32 cuda tensor of x's rank.  Frames outside the
    range count as zero, so the cut costs no copy of a resident tensor."""
    torch = _torch()
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be >= 1")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    a, n, ch, rank = _as_device(x)
    stop = n if stop is None else min(int(stop), n)
    start = int(start)
    if not 0 <= start < stop:
        raise ValueError("resample_poly needs a non-empty range inside the signal")
    ln = stop - start
    is_tensor = isinstance(a, torch.Tensor)
    if up == down:
        part = a[start:stop]
        return part.clone() if is_tensor else _upload(part)
    if not _in_limits(up, down) or not 1 <= ch <= MAX_CH:
        raise ValueError(f"up={up}, down={down}, channels={ch}: {_limits_text()}")
    if not is_tensor:  # a host array: only the range is uploaded
        a, n, start = _upload(a[start:stop]), ln, 0
    h = torch.from_numpy(taps(up, down).copy()).cuda()
    m = n_out(ln, up, down)
    out = torch.empty((m,) if rank == 1 else (m, ch), dtype=torch.float32, device="cuda")
    check(lib().tomatis_resample_poly(ptr(a), n, start, ln, ch, up, down, ptr(h), h.numel(),
                                      ptr(out), stream_handle()), "resample_poly")
    return out


def resample_to(x, sr: int, target_sr: int = 48000, start: int = 0, stop=None):
    """Frames [start, stop) of x at ``sr`` resampled to ``target_sr``."""
    if not supported(sr, target_sr):
        up, down = ratio(sr, target_sr)
        raise ValueError(f"sr={sr}, target_sr={target_sr} (up={up}, down={down}): "
                         f"{_limits_text()}")
    return resample_poly(x, int(target_sr), int(sr), start, stop)


__all__ = ["taps", "resample_poly", "resample_to", "supported", "ratio", "n_out",
           "outputs_per_workgroup", "lds_words"]
