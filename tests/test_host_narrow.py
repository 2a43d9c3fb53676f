"""BandEd score-only in two passes on the host: launch_banded_narrow / launch_banded_probe and the policy around them, built
with g++ against the fake HIP runtime of tests/native/hip_stub (as tests/test_host_sanitizers.py builds the host layer)
under AddressSanitizer + UBSan, driven by tests/native/narrow_host.cpp through the C-ABI.  No GPU."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_two_pass_launches_and_policy_under_address_and_ub_sanitizers(tmp_path):
    exe = build_host("narrow_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SCORE_NARROW", "QE_STUB_BOUND"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "narrow_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
