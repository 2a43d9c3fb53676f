"""All-occurrences runs on the host: the argument rules, the QUICKED_UNIMPLEMENTED cases, the limits of max_hits and of its
product with the pairs, the flow of run_search_hits in both kernel forms, batches with empty pairs, the getters' rules after
other runs and a reload between runs -- the library's host layer built with g++ against the fake HIP runtime of
tests/native/hip_stub (as tests/test_host_search.py builds it; the host stand-ins of k_search_hits, k_hits_expand and
k_hits_finish in qe_stages.hip run the recurrence of qe_search.h) under AddressSanitizer + UBSan, driven by
tests/native/search_hits_host.cpp through the C-ABI.  A stand-alone program; no GPU."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


def test_search_hits_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    exe = build_host("search_hits_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SEARCH_FORM", "QE_TAGS_WAVE", "QE_FORMAT_WAVE", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "search_hits_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
