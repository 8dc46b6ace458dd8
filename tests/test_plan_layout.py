"""CPU: the processor plan's layout and ownership (csrc/tm_plan.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer (tools/plan_check.cpp).

The plan unit is host code only, so the check program links it with a fake
runtime over malloc (no HIP runtime, no GPU) and reads back what each plan
uploads: the cut of every stream into interior and edge runs, frame by frame
against what the fused kernel's interior loop assumes; the fused limiter's
flushes per chunk and run span against a brute-force count with the kernel's
own chunk rule; chunk descriptors, level blocks, gate / alpha segments, leaf and
group prefixes and min-hold offsets.  Every plan is destroyed, creation is
repeated with each allocation failing in turn, invalid streams are refused, and
LeakSanitizer reports at exit.  The build aborts on the first sanitizer report.
"""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm", *sorted(glob.glob("/opt/rocm-*"))):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def test_plan_layout_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    inc = _hip_include()
    if inc is None:
        pytest.skip("no HIP headers")
    exe = str(tmp_path / "plan_check")
    # (-Wno-subobject-linkage: tm_layout.h keeps the kernels' work-item structs
    # in an unnamed namespace, and the plan holds buffers of them)
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-subobject-linkage",
           "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tomatis_audio_processor_amd", "csrc", "tm_plan.cpp"),
           os.path.join(ROOT, "tools", "plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower():
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    tail = (r.stderr or "")[-3000:]
    assert r.returncode == 0, tail
    assert "failures 0" in tail, tail
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, tail
