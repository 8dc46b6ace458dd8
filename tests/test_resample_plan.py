"""CPU: the audio resampler's index arithmetic (csrc/tm_resample_plan.h, used by
tm_resample.hip k_rs_poly and tomatis_resample_poly) under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/resample_plan_check.cpp), and the Python
mirror of its plan (``resample.outputs_per_workgroup`` / ``lds_words``) against
the plans that program prints.

The header is host and device code with no HIP in it, so the check program is
built with the host compiler alone: no GPU, and nothing sanitized but that
program.  It checks the tile plan over the whole supported domain (every
reduced ratio with max(up, down) <= 512 and down <= 8 up, 1 to 8 channels),
replays the kernel's LDS reads element by element against the statement in
64-bit integers for a list of plans, custom tap counts and the tile just under
the 2^31 - 1 limit among them, and holds the entry point's argument rule to the
expectations of test_gpu_resample.py::test_entry_point_guards.  The GPU tests
take every tile-edge length from the Python mirror: the comparison here is
what makes those lengths edges of the C plan.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (ratio, channels) a GPU test derives a length from: the default filter
# of each ratio of test_gpu_resample.py and test_gpu_resample_paths.py ...
DEFAULT = [(160, 147), (80, 147), (40, 147), (1, 2), (1, 4), (3, 2), (2, 1), (320, 147), (6, 1),
           (3, 1), (512, 511), (1, 8), (4, 7), (2, 3)]
# ... and the custom filters of test_gpu_resample_paths.py::test_custom_taps_*
CUSTOM = [(3, 2, 1), (3, 2, 5), (5, 3, 3), (7, 5, 13), (1, 2, 7), (2, 3, 15), (160, 147, 159),
          (160, 147, 161), (1, 2, 41), (160, 147, 3201)]
CUSTOM_CH = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def checker_output(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rs_plan") / "resample_plan_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           os.path.join(ROOT, "tools", "resample_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower():
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def test_resample_plan_sanitizers(checker_output):
    r = checker_output
    tail = (r.stderr or "")[-3000:]
    assert r.returncode == 0, tail
    lines = r.stdout.splitlines()
    assert lines and lines[-1] == "failures 0", (lines[-3:], tail)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, tail
    # the whole-domain pass ran: the count of reduced ratios inside the limits, times 8
    import math
    pairs = sum(1 for u in range(1, 513) for d in range(1, 513)
                if u != d and d <= 8 * u and math.gcd(u, d) == 1)
    assert f"whole domain: {8 * pairs} plans" in lines


def test_python_plan_is_the_c_plan(checker_output):
    from tomatis_audio_processor_amd import resample
    plans = {}
    for ln in checker_output.stdout.splitlines():
        if ln.startswith("plan "):
            up, down, n_taps, ch, T, W, stage, tab = map(int, ln.split()[1:])
            plans[(up, down, n_taps, ch)] = (T, W, stage, tab)
    want = [(u, d, 20 * max(u, d) + 1, ch) for u, d in DEFAULT for ch in range(1, 9)]
    want += [(u, d, n, ch) for u, d, n in CUSTOM for ch in CUSTOM_CH]
    assert set(want) <= set(plans), sorted(set(want) - set(plans))
    for (up, down, n_taps, ch), (T, W, stage, tab) in plans.items():
        key = (up, down, n_taps, ch)
        assert resample.outputs_per_workgroup(up, down, ch, n_taps) == T, key
        assert resample.lds_words(up, down, ch, n_taps) == stage + tab, key
        if n_taps == 20 * max(up, down) + 1:  # the default filter: n_taps left out
            assert resample.outputs_per_workgroup(up, down, ch) == T, key
            assert resample.lds_words(up, down, ch) == stage + tab, key
        # the printed line agrees with itself: W frames of ch words and up to 3 in front
        K4 = -(-(-(-n_taps // up)) // 4) * 4
        assert W == (up - 1 + down * (T - 1)) // up + K4, key
        assert stage == (3 + W * ch + 3) // 4 * 4 and 4 * (stage + tab) <= 64 * 1024, key
