"""Mismatch-only panel runs (QUICKED_PANEL_NO_INDELS) on the host: every refusal of the contract with nothing launched -- the
QUICKED_ERROR rules of the two runs first, the bit as an unknown bit of the other runs, QUICKED_UNIMPLEMENTED beside CIGARS, TAILS
or HEADS, with sync == 0 (also on a batch object whose queue is switched on), with a member over 256 bases and with check != 0 --,
the groups of tests/golden/panel_noindels_cases.json through quicked_batch_run_panel (with and without the matrix) and
quicked_batch_run_panel_all under the two IUPAC flags, PREFIX and INFIX, QE_PANEL_SLICES unset, 1 and huge, caps of 1, 2 and the
fixture's, and every getter the contract names: the library's host layer built with g++ against the fake HIP runtime of
tests/native/hip_stub under AddressSanitizer + UBSan, exactly as tests/test_host_panel_scan.py builds it, driven by
tests/native/panel_noindels_host.cpp through the C-ABI.  The expectations are tests/panel_noindels_lib.py's, handed over in a
file.  A stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import panel_noindels_lib as N
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_panel_noindels_cases", os.path.join(ROOT, "tests", "golden", "make_panel_noindels_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_panel_noindels_runs_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    G = _cases()
    groups = G.load()
    N.cases_file(str(tmp_path / "cases"), [groups[name] for name in ("lengths", "homopolymer", "indels", "single", "bytes", "panel130", "wave65")], G.CAP, (N.IUPAC, N.IUPAC_PATTERN))
    exe = build_host("panel_noindels_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_noindels_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
