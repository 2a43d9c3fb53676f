"""Alignment tags on the host: format_segments / fetch_alignments with the tag arrays and the MD pool, the getters' rules and
NO_CIGAR, built with g++ against the fake HIP runtime of tests/native/hip_stub (as tests/test_host_sanitizers.py builds the
host layer; the tag kernels' host stand-ins of qe_stages.hip run the walker of qe_tags.h) under AddressSanitizer + UBSan,
driven by tests/native/tags_host.cpp through the C-ABI; the same program drives the validator's entry points, whose host stand-ins
run the walk of qe_check.h.  No GPU."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


def test_tags_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    exe = build_host("tags_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_TAGS_WAVE", "QE_FORMAT_WAVE", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "tags_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
