"""Flagged search runs (QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN) on the host: the argument rules, the
QUICKED_UNIMPLEMENTED cases, sync and queued flagged runs in both kernel forms with true answers (the host stand-ins of the
plane producers are the scalar code of qe_iupac.h), flagged and unflagged runs in turn with a reload in between, a packed
PLANES3 batch and quicked_batch_run_search_all with a cap of 1 -- the library's host layer built with g++ against the fake
HIP runtime of tests/native/hip_stub under AddressSanitizer + UBSan, exactly as tests/test_host_search.py builds it, driven
by tests/native/search_iupac_host.cpp through the C-ABI.  The expectations are the brute force's (tests/iupac_lib.py),
handed over in a file.  A stand-alone program; no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import iupac_lib as I
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_iupac_cases", os.path.join(ROOT, "tests", "golden", "make_search_iupac_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pairs():
    """small cases one can read, the named ones, patterns of every block count (1, 2, 3-4, more), empty sequences; twice:
    the second half is what the batch is reloaded with"""
    G = _cases()
    hand = [(b"ACGT", b"TTACNTTT"), (b"AC-GT", b"ttAC-GTtt"), (b"acgyn", b"TTACGCGTT"), (b"RRRR", b"YYYYYYYY"), (b"", b"ACGT"), (b"ACGT", b"")]
    grid = [c for c in G.grid_cases() if len(c[1]) in (65, 130)]
    first = hand + G.named_cases() + grid[0::2][:24] + G.random_cases()[:30] + G.tie_cases()[1:30:2]
    second = G.random_cases()[30:70] + grid[1::2][:24] + [(b"", b"A"), (b"NNNN", b"ACGTACGT")] + G.tie_cases()[31:50:2]
    if len(first) > len(second):
        second += G.random_cases()[70:70 + len(first) - len(second)]
    return first + second[:len(first)]


def test_expectations_a_reader_can_check():
    assert I.locate(b"ACGT", b"TTACNTTT", I.INFIX, I.IUPAC) == (0, 2, 6) and I.locate(b"ACGT", b"TTACNTTT", I.INFIX, I.IUPAC_PATTERN) == (1, 2, 6)
    assert I.locate(b"AC-GT", b"ttAC-GTtt", I.INFIX, I.IUPAC) == (1, 2, 7)
    assert I.locate(b"RRRR", b"YYYYYYYY", I.INFIX, I.IUPAC) == (4, 0, 1)


def test_flagged_search_host_side_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    lines = []
    for p, t in pairs():
        row = [p.decode() or ".", t.decode() or "."]
        for flag in (I.IUPAC, I.IUPAC_PATTERN):
            for mode in (I.PREFIX, I.INFIX):
                row += [str(v) for v in (I.locate(p, t, mode, flag) if p and t else (-1, -1, -1))]
        for flag in (I.IUPAC, I.IUPAC_PATTERN):
            occ = I.occurrences(p, t, I.INFIX, flag, 2) if p and t else []
            row += [str(len(occ))] + [str(v) for v in (occ[0] if occ else (-1, -1, -1))]
        lines.append(" ".join(row))
    (tmp_path / "cases").write_text("\n".join(lines) + "\n")
    exe = build_host("search_iupac_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_SEARCH_FORM", "QE_TAGS_WAVE", "QE_FORMAT_WAVE", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "search_iupac_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
