"""The pruning threshold of a fitted first pass (QE_NARROW_PRUNE) on the host: k_narrow's host rendering with the thresholds,
the forced switch and the window rule of the policy (one report: none; two equal reports: r^; a stale ring: the fitted cutoff;
forgotten after 16 reports), built with g++ against the fake HIP runtime of tests/native/hip_stub under AddressSanitizer +
UBSan (as tests/test_host_narrow_fit.py builds the same layer), driven by tests/native/narrow_prune_host.cpp through the
C-ABI.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pruning_threshold_and_its_policy_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "narrow_prune_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unused-parameter",
           "-Wno-class-memaccess", "-DQE_KERNELS_HEADER=\"qe_kernels_stub.h\"", "-I" + os.path.join(NATIVE, "hip_stub"),
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-x", "c++", os.path.join(CSRC, "qe_driver.hip"), os.path.join(CSRC, "qe_capi.cpp"), os.path.join(CSRC, "qe_hostpack.cpp"),
           os.path.join(NATIVE, "narrow_prune_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SCORE_NARROW", "QE_NARROW_FIT", "QE_NARROW_PRUNE", "QE_STUB_BOUND"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "narrow_prune_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
