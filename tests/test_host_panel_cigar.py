"""Occurrence alignments (QUICKED_PANEL_CIGARS) on the host: every argument rule with nothing launched (the bit on
quicked_batch_run_panel, with QUICKED_PANEL_MATRIX, every refusal of the two runs), the getters' rules around runs without the bit,
other kinds of run and a reload, and true strings on the named set of tests/golden/panel_cigar_cases.json under the two IUPAC
flags -- quicked_batch_run_panel_all (PREFIX, INFIX) and quicked_batch_run_panel_scan (windows 64 and 0), styles 0 / 1 / 2, caps
of 1, 2 and 64, QE_PANEL_ALIGN_WS_KB unset and 1 -- with the results of the run without the bit unchanged by it: the library's host
layer built with g++ against the fake HIP runtime of tests/native/hip_stub under AddressSanitizer + UBSan, exactly as
tests/test_host_panel_scan.py builds it, driven by tests/native/panel_cigar_host.cpp through the C-ABI.  The expectations are
tests/panel_cigar_lib.py's, handed over in a file.  A stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import panel_cigar_lib as PC
import panel_hits_lib as P
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_panel_cigar_cases", os.path.join(ROOT, "tests", "golden", "make_panel_cigar_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_panel_cigars_run_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    s = _cases().load()["named"]
    PC.cases_file(str(tmp_path / "cases"), s, (P.PREFIX, P.INFIX), (P.IUPAC, P.IUPAC_PATTERN), ("own",))
    exe = build_host("panel_cigar_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_cigar_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
