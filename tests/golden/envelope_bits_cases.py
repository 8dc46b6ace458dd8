"""Cases of tests/golden/envelope_ds_bits.npz (tools/make_envelope_bits_goldens.py):
the output bits of ``tomatis_align_envelope`` and ``tomatis_align_envelope_mean_first``
as the library with two decimators computed them (through its kernel for up == 1,
removed since), at values of ``down`` where the one polyphase kernel keeps that
kernel's summation order: one thread per output, which holds up to down = 53.

Stereo white noise of 600 down + 17 frames (601 outputs: two full tiles of 256
and a ragged third) at down 2, 3, 24, 48 and 53, and at down 24 the sub-range
1237..7001 of a resident 9000-frame signal, each in both mean orders."""
import zlib

import numpy as np

from tests.stft_ref import white

DOWNS = [2, 3, 24, 48, 53]
FIXTURE = "envelope_ds_bits"


def _cases():
    for down in DOWNS:
        n = 600 * down + 17
        for mean_first in (False, True):
            yield dict(key=f"d{down}_{'first' if mean_first else 'last'}", seed=8800 + down,
                       down=down, n=n, start=0, stop=n, mean_first=mean_first)
    for mean_first in (False, True):
        yield dict(key=f"d24_sub_{'first' if mean_first else 'last'}", seed=8900, down=24,
                   n=9000, start=1237, stop=7001, mean_first=mean_first)


BITS_CASES = list(_cases())


def make_input(c):
    """-> (float32 [n, 2], CRC-32 of its bytes)."""
    x = white(c["seed"], c["n"], 2)
    return x, zlib.crc32(np.ascontiguousarray(x).tobytes())


def run_entry_point(c, x):
    """The case through the C entry point of its mean order, called directly on
    the whole resident ``x``: -> (output bits as uint32, the float64 mean)."""
    import torch
    from tomatis_audio_processor_amd import align
    from tomatis_audio_processor_amd._lib import ALIGN_MEAN_DOUBLES, check, lib, ptr, stream_handle
    down, ln = c["down"], c["stop"] - c["start"]
    xd = torch.from_numpy(x).cuda()
    taps = torch.from_numpy(align._taps(down)).cuda()
    out = torch.empty(-(-ln // down), dtype=torch.float32, device="cuda")
    mean = torch.empty(ALIGN_MEAN_DOUBLES, dtype=torch.float64, device="cuda")
    fn = lib().tomatis_align_envelope_mean_first if c["mean_first"] else lib().tomatis_align_envelope
    check(fn(ptr(xd), c["n"], c["start"], ln, down, ptr(taps), taps.numel(), ptr(out), ptr(mean),
             stream_handle()), "align_envelope")
    return out.cpu().numpy().view(np.uint32), float(mean[0].item())
