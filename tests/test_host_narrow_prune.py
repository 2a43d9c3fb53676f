"""The pruning threshold of a fitted first pass (QE_NARROW_PRUNE) on the host: k_narrow's host rendering with the thresholds,
the forced switch and the window rule of the policy (one report: none; two equal reports: r^; a stale ring: the fitted cutoff;
forgotten after 16 reports), built with g++ against the fake HIP runtime of tests/native/hip_stub under AddressSanitizer +
UBSan (as tests/test_host_narrow_fit.py builds the same layer), driven by tests/native/narrow_prune_host.cpp through the
C-ABI.  No GPU."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pruning_threshold_and_its_policy_under_address_and_ub_sanitizers(tmp_path):
    exe = build_host("narrow_prune_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SCORE_NARROW", "QE_NARROW_FIT", "QE_NARROW_PRUNE", "QE_STUB_BOUND"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "narrow_prune_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
