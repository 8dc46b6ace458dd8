#!/usr/bin/env python3
"""Generate ``tests/golden/envelope_ds_bits.npz``: the output bits and the means
of ``tomatis_align_envelope`` and ``tomatis_align_envelope_mean_first`` on the
cases of ``tests/golden/envelope_bits_cases.py``, as computed by a library built
from the commit BEFORE the two decimators of ``tm_align.hip`` became one (the
last one whose ``tomatis_align_envelope`` ran a kernel of its own for up == 1).

Needs an MI355X and that library: build it from a worktree of that commit with
``python -m tomatis_audio_processor_amd.build --out /path/libtomatis_parent.so``
and point ``TOMATIS_HIP_LIB`` at it.  The entry points are called directly, so
the Python of this tree does not matter.  Per case the fixture holds the
``uint32`` view of the output, the float64 mean and the CRC-32 of the input
bytes; nothing else.  ``tests/test_gpu_align.py`` holds the current kernel to
these bits: with the old kernel gone, a comparison of the two paths would
compare the kernel with itself.

Usage:  TOMATIS_HIP_LIB=/path/libtomatis_parent.so python tools/make_envelope_bits_goldens.py
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from tests.golden.envelope_bits_cases import BITS_CASES, FIXTURE, make_input, run_entry_point  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", FIXTURE + ".npz"))
    a = ap.parse_args()
    if "TOMATIS_HIP_LIB" not in os.environ:
        raise SystemExit("set TOMATIS_HIP_LIB to a library of the last commit with two decimators")
    from tomatis_audio_processor_amd import _lib
    print(f"library: {_lib.lib_path()}")
    fx = {}
    for c in BITS_CASES:
        x, crc = make_input(c)
        bits, mean = run_entry_point(c, x)
        again, _ = run_entry_point(c, x)
        assert np.array_equal(bits, again), (c["key"], "run-to-run")
        fx[c["key"] + "_bits"] = bits
        fx[c["key"] + "_mean"] = np.array(mean, np.float64)
        fx[c["key"] + "_crc"] = np.array(crc, np.uint32)
        print(f"{c['key']:16s} {len(bits):5d} outputs  mean {mean:.17g}  crc {crc:08x}")
    np.savez_compressed(a.out, **fx)
    size = os.path.getsize(a.out)
    assert size < 65536, size
    print(f"{a.out}: {size} bytes")


if __name__ == "__main__":
    main()
