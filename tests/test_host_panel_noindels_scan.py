"""The windowed mismatch-only panel run (quicked_batch_run_panel_scan_no_indels) on the host: every QUICKED_ERROR and
QUICKED_UNIMPLEMENTED rule with nothing launched (the scan's, the bits that are unknown to it, PREFIX, QUICKED_PANEL_CIGARS,
sync == 0 also on a batch switched on for queued runs, a member over 256 bases, check != 0, the 2^26 rules), the getters' rules
around the other kinds of run, results cleared by a reload, and true answers on groups of
tests/golden/panel_noindels_scan_cases.json under the two IUPAC flags -- the definition's lists, the model's block steps and the
flagged quicked_batch_run_panel_all's results on the same batch -- with caps of 1, 2 and 4096, windows of 64, 128, 192, 4096 and
the library's and QE_PANEL_SLICES unset, 1 and huge: the library's host layer built with g++ against the fake HIP runtime of
tests/native/hip_stub under AddressSanitizer + UBSan, exactly as tests/test_host_panel_scan.py builds it, driven by
tests/native/panel_noindels_scan_host.cpp through the C-ABI.  The fake runtime's k_pack writes no planes, so an unflagged run
is held to its statuses and the shape of its results here, and to the definition in tests/test_panel_noindels_scan_cpu.py and
on the GPU.  A stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import panel_noindels_lib as N
import panel_noindels_scan_lib as S
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("bytes", "staircase24", "staircase129", "copies64", "copies256", "plateau65", "polyA", "short129", "bounds")


def _cases():
    spec = importlib.util.spec_from_file_location("make_panel_noindels_scan_cases", os.path.join(ROOT, "tests", "golden", "make_panel_noindels_scan_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_panel_noindels_scan_runs_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    by = {g["name"]: g for g in _cases().load()}
    groups = []
    for name in GROUPS:
        g = by[name]
        res = {f: [N.text_hits(t, g["panel"], g["bounds"], N.INFIX, f) for t in g["texts"]] for f in (N.IUPAC, N.IUPAC_PATTERN)}
        if 0 in g["results"] and not any(set(t.upper()) - set(b"ACGT") for t in g["texts"] + g["panel"]):
            assert res[N.IUPAC] == g["results"][0] and res[N.IUPAC_PATTERN] == g["results"][0]      # plain bases: the three equalities agree
        groups.append(dict(g, results=res))
    S.cases_file(str(tmp_path / "cases"), groups)
    exe = build_host("panel_noindels_scan_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_noindels_scan_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
