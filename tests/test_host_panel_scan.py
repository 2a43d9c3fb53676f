"""Windowed panel runs (quicked_batch_run_panel_scan) on the host: every QUICKED_ERROR and QUICKED_UNIMPLEMENTED rule with nothing
launched (run_panel_all's, the window's, PREFIX, the 2^26 rule with a forced window and window == 0 accepted where a forced one is
refused), the getters' rules around the other kinds of run, results cleared by a reload, and true answers on the boundary set of
tests/golden/panel_scan_cases.json under the two IUPAC flags -- the fixture's lists and quicked_batch_run_panel_all's results on
the same batch -- with caps of 1, 2 and 64, windows of 64, 128 and the library's, QE_PANEL_SLICES = 1, 2 and a huge value and a
1 KiB QE_PANEL_HITS_RAW_KB: the library's host layer built with g++ against the fake HIP runtime of tests/native/hip_stub under
AddressSanitizer + UBSan, exactly as tests/test_host_panel_hits.py builds it, driven by tests/native/panel_scan_host.cpp through
the C-ABI.  The expectations are tests/panel_hits_lib.py's, handed over in a file.  A stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import panel_hits_lib as P
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_panel_scan_cases", os.path.join(ROOT, "tests", "golden", "make_panel_scan_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_panel_scan_runs_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    s = _cases().load()["windows"]
    P.cases_file(str(tmp_path / "cases"), s, (P.INFIX,), (P.IUPAC, P.IUPAC_PATTERN))
    exe = build_host("panel_scan_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_scan_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
