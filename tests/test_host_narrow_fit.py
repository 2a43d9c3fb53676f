"""The fitted first pass of BandEd score-only in two passes on the host: k_narrow's host rendering with the fit's group rule,
the forced switch and the learning policy, built with g++ against the fake HIP runtime of tests/native/hip_stub under
AddressSanitizer + UBSan (as tests/test_host_narrow.py builds the same layer), driven by tests/native/narrow_fit_host.cpp
through the C-ABI.  No GPU."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fitted_first_pass_and_its_policy_under_address_and_ub_sanitizers(tmp_path):
    exe = build_host("narrow_fit_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SCORE_NARROW", "QE_NARROW_FIT", "QE_STUB_BOUND"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "narrow_fit_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
