"""All-occurrences panel runs (quicked_batch_run_panel_all) on the host: every QUICKED_ERROR and QUICKED_UNIMPLEMENTED rule with
nothing launched, the getters' rules before and after each other kind of run, results cleared by a reload, true answers on the
named set under the two IUPAC flags with caps of 1, 2 and 64 (the host stand-ins of the kernels are the kernels' own source,
qe_panel.h, and the stand-in of k_pack_iupac is the scalar packer), QE_PANEL_SLICES = 1, 2 and a huge value, and a tiny
QE_PANEL_HITS_RAW_KB that forces the slice count down -- the library's host layer built with g++ against the fake HIP runtime
of tests/native/hip_stub under AddressSanitizer + UBSan, exactly as tests/test_host_search_panel.py builds it, driven by
tests/native/panel_hits_host.cpp through the C-ABI.  The expectations are tests/panel_hits_lib.py's, handed over in a file.  A
stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import panel_hits_lib as P
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_panel_hits_cases", os.path.join(ROOT, "tests", "golden", "make_panel_hits_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_panel_all_runs_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    s = _cases().load()["named"]
    P.cases_file(str(tmp_path / "cases"), s, (P.PREFIX, P.INFIX), (P.IUPAC, P.IUPAC_PATTERN))
    exe = build_host("panel_hits_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_hits_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
