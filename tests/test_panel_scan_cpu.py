"""Windowed panel search (quicked_batch_run_panel_scan), the part that needs no GPU: the public surface, what the boundary
fixture holds, and the core of quicked_amd/csrc/qe_panel.h / qe_search.h -- SearchHitScanOf with an owned range,
panel_window_hits and the count / expand bodies: the source k_panel_scan and its small kernels run per lane -- compiled with g++
as a stand-alone program (tests/native/panel_scan_cpu.cpp), plain and under ASan + UBSan, and compared with the definition
(tests/panel_hits_lib.py) and with the unwindowed path on the boundary set of tests/golden/panel_scan_cases.json and on the INFIX
cases of tests/golden/panel_hits_cases.json: windows of 64, 128, 192 and 4096 columns, 1, 2 and K slices, caps of 1, 2 and
4096, both equalities and all three flag settings."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_hits_lib as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
MODES = (PH.INFIX,)
FLAGS = (0, PH.IUPAC, PH.IUPAC_PATTERN)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_hits_cases")
GS = _load("make_panel_scan_cases")


@pytest.fixture(scope="module")
def sets():
    out = dict(G.load())
    out.update(GS.load())
    return out


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "quicked_batch_run_panel_scan(" in flat
    for phrase in ("it leaves exactly the results quicked_batch_run_panel_all leaves for the same batch, panel, mode, bounds and max_hits, whatever `window` is",
                   "a scan run is a run of their kind",
                   "warm-up and run-out columns included",
                   "Otherwise a multiple of 64 that is at least 64",
                   "(window slots of the batch = the sum of ceil(n / window) over the texts) x max_hits above 2^26",
                   "the base mode QUICKED_SEARCH_PREFIX",
                   "sync == 0", "a batch configured with check != 0",
                   "Not built: a cap above 4096 per text, queued runs, members over 256 bases, alignments of occurrences"):
        assert phrase in flat, phrase


def test_refusals_without_a_device():
    from quicked_amd import capi
    lib = capi.lib()
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel_scan(None, PH.INFIX, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 64, 1) == capi.QUICKED_ERROR
    assert callable(capi.ResidentBatch.run_panel_scan)
    assert "quicked_batch_run_panel_scan" in capi.EXPORTS


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_the_record_is_the_brute_force(sets):
    """a fixed sample of the recorded lists, recomputed live (the generator computed every list the same way)"""
    rng = np.random.default_rng(7)
    s = sets["windows"]
    n = len(s["texts"])
    assert set(s["hits"]) == {(PH.INFIX, f, c) for f in FLAGS for c in GS.CONFS}
    for (mode, flag, conf), rec in s["hits"].items():
        assert len(rec) == n
        for i in rng.integers(0, n, 3):
            assert rec[int(i)] == PH.text_hits(s["texts"][int(i)], s["panel"], GS.bounds_of(s, conf), mode, flag), (flag, conf, int(i))


def test_the_set_holds_what_it_is_for(sets):
    """the generator asserts the constructions in full; here what can be read off the record"""
    s = sets["windows"]
    own = s["hits"][(PH.INFIX, 0, "own")]
    assert {len(t) for t in s["texts"]} >= {0, 1, 63, 64, 65, 127, 128, 129} and max(len(t) for t in s["texts"]) <= 700
    assert {len(q) for q in s["panel"]} >= {1, 61, 124, 256} and s["bounds"][2] > len(s["panel"][2])
    for d in (-1, 0, 1, 2):                                          # exact plants ending at c + d
        assert sum(1 for h in own for o in h if o[0] in (0, 1) and o[3] == 0 and o[2] > 2 and (o[2] - d) % 64 == 0) >= 8, d
    for p in (3, 4):                                                 # score k over a stretch of m + k = 64 / 128 columns, ending at c and c + 1
        k, m = s["bounds"][p], len(s["panel"][p])
        ends = {o[2] % 64 for h in own for o in h if o[0] == p and o[3] == k and o[2] - o[1] == m + k}
        assert m + k in (64, 128) and ends >= {0, 1}, (p, ends)
    assert any(o[0] == 5 and o[3] == 0 and len(t) - o[2] >= 3 * 64 and t.endswith(b"A" * 200) for t, h in zip(s["texts"], own) for o in h)
    assert set(b"RYN") <= set(s["panel"][8]) and any(b"N" in t for t in s["texts"])
    assert any(len(h) > 64 for h in own)
    assert sum((len(t) + 63) // 64 for t in s["texts"]) * 4096 <= 2**26


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the panel core for the host")
    exe = os.path.join(tmp, f"panel_scan_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_scan_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_scan"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("name", ["windows", "named", "random"])
def test_panel_scan_core_equals_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    PH.cases_file(path, sets[name], MODES, FLAGS)
    for exe in programs:
        out = _run(exe, "cases", path)
        assert re.search(r"cases ok (\d+)", out) and int(re.search(r"cases ok (\d+)", out).group(1)) > 1000, out
