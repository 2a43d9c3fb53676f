"""The windowed mismatch-only panel run (quicked_batch_run_panel_scan_no_indels), the part that needs no GPU: the public surface,
what the boundary fixture holds, the window rule by plain loops (tests/panel_noindels_scan_lib.py) against the definition, and
the core of quicked_amd/csrc/qe_panel_ham.h / qe_panel.h -- PanelHamScanOf with an owned range, panel_ham_window_hits and the
count / expand bodies: the source k_panel_ham_scan and its small kernels run per lane -- compiled with g++ as a stand-alone
program (tests/native/panel_noindels_scan_cpu.cpp), plain and under ASan + UBSan, on the boundary set of
tests/golden/panel_noindels_scan_cases.json and on the INFIX cases of tests/golden/panel_noindels_cases.json: windows of 64, 128,
192 and 4096 columns, 1, 2 and K slices, caps of 1, 2 and 4096, all three flag settings, the block steps against the model."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_noindels_lib as N
import panel_noindels_scan_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
FLAGS = (0, N.IUPAC, N.IUPAC_PATTERN)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GS = _load("make_panel_noindels_scan_cases")
GN = _load("make_panel_noindels_cases")


def infix_groups_of_the_unwindowed_fixture():
    """panel_noindels_cases.json's groups with the uncapped INFIX lists (its record keeps a text's first 8)"""
    out = []
    for g in GN.load().values():
        res = {f: [N.text_hits(t, g["panel"], g["bounds"], N.INFIX, f) for t in g["texts"]] for f in FLAGS}
        for f in FLAGS:
            rec = g["results"][(N.INFIX, f)]
            assert [len(h) for h in res[f]] == rec["found"] and [h[:GN.CAP] for h in res[f]] == rec["occ"], (g["name"], f)
        out.append({"name": g["name"], "panel": g["panel"], "bounds": g["bounds"], "texts": g["texts"], "results": res})
    return out


@pytest.fixture(scope="module")
def boundary():
    return GS.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "quicked_batch_run_panel_scan_no_indels(" in flat
    for phrase in ("it leaves exactly what quicked_batch_run_panel_all leaves for the same batch, panel, mode | QUICKED_PANEL_NO_INDELS, bounds and max_hits, whatever `window` is",
                   "text_start = text_end - m",
                   "the bit in `mode` is accepted and means nothing more",
                   "[0] is the block steps really walked",
                   "[1] .. [7] are 0",
                   "QUICKED_PANEL_MATRIX, QUICKED_PANEL_TAILS and QUICKED_PANEL_HEADS (unknown bits of the scan)",
                   "the base mode QUICKED_SEARCH_PREFIX; QUICKED_PANEL_CIGARS; sync == 0",
                   # what the header said before stays said
                   "QUICKED_ERROR, nothing launched: the bit on quicked_batch_run_panel_scan, _run_search and _run_search_all"):
        assert phrase in flat, phrase


def test_refusals_without_a_device():
    from quicked_amd import capi
    lib = capi.lib()
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel_scan_no_indels(None, N.INFIX, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 64, 1) == capi.QUICKED_ERROR
    assert callable(capi.ResidentBatch.run_panel_scan_no_indels)
    assert "quicked_batch_run_panel_scan_no_indels" in capi.EXPORTS


# ---- the fixture and the window rule -----------------------------------------------------------------------------------
def test_the_record_is_the_brute_force(boundary):
    """a fixed sample of the recorded lists, recomputed live (the generator computed every list the same way)"""
    rng = np.random.default_rng(11)
    for g in boundary:
        for flag, rec in g["results"].items():
            assert len(rec) == len(g["texts"])
            for i in rng.integers(0, len(g["texts"]), 2):
                assert rec[int(i)] == N.text_hits(g["texts"][int(i)], g["panel"], g["bounds"], N.INFIX, flag), (g["name"], flag, int(i))


def test_the_set_holds_what_it_is_for(boundary):
    """the generator asserts the constructions and conditions (a) - (c) in full; here what can be read off the record"""
    by = {g["name"]: g for g in boundary}
    assert {len(q) for g in boundary for q in g["panel"]} >= set(GS.LENS)
    assert {len(t) for g in boundary for t in g["texts"]} >= {0, 23, 24, 63, 64, 65, 127, 128, 129, 130}
    assert max(len(t) for g in boundary for t in g["texts"]) <= 1100
    ends = {o[2] - c for g in boundary if g["name"].startswith("copies") for h in g["results"][0] for o in h for c in (64, 128, 192) if abs(o[2] - c) <= 2}
    assert ends >= {-1, 0, 1, 2}
    assert any(len(h) > 64 for h in by["bounds"]["results"][0])
    assert by["bounds"]["bounds"][0] > len(by["bounds"]["panel"][0]) and N.INT32_MAX in by["bounds"]["bounds"]
    assert set(by["bytes"]["results"]) == set(FLAGS) and any(set(t) == {ord("N")} for t in by["bytes"]["texts"])
    assert any(len(q) > len(t) > 0 for g in boundary for q in g["panel"] for t in g["texts"])
    assert sum((len(t) + 63) // 64 for g in boundary for t in g["texts"]) * 4096 <= 2**26


@pytest.mark.parametrize("window", [64, 128, 192, 4096, 0])
def test_window_rule_equals_the_definition(boundary, window):
    for g in boundary:
        for flag, rec in g["results"].items():
            for t, want in zip(g["texts"], rec):
                assert S.text_hits(t, g["panel"], g["bounds"], flag, window) == sorted(want), (g["name"], flag, window)


def test_wrong_window_rules_are_told_apart(boundary):
    """conditions (b) and (c) on a sample: the staircases separate both wrong rules from the definition at both windows"""
    g = next(g for g in boundary if g["name"] == "staircase24")
    for window in (64, 128):
        for wrong in ("prev", "runout"):
            differ = sum(S.text_hits(t, g["panel"], g["bounds"], 0, window, wrong) != want for t, want in zip(g["texts"], g["results"][0]))
            assert 4 * differ >= len(g["texts"]), (window, wrong, differ)


def test_steps_of_one_window_are_the_unwindowed_runs():
    """one slot per text walks every start once: the flagged run_panel_all's count"""
    panel, texts = [b"ACGTACGTAC", b"A" * 70, b"C" * 129], [b"ACGT" * 40, b"A" * 64, b"ACG", b"C" * 300]
    assert S.block_steps(texts, panel, [1, 1, 1], 0, 0) == N.block_steps(texts, panel, N.INFIX)
    assert S.block_steps(texts, panel, [1, 1, 1], 0, 4096) == N.block_steps(texts, panel, N.INFIX)
    assert S.block_steps(texts, panel, [1, 1, 1], 0, 64) > N.block_steps(texts, panel, N.INFIX)       # one lead-in start per later slot, and the run-outs


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the panel core for the host")
    exe = os.path.join(tmp, f"panel_noindels_scan_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_noindels_scan_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_noindels_scan"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("name", ["boundary", "unwindowed"])
def test_panel_noindels_scan_core_equals_the_definition(programs, boundary, tmp_path, name):
    path = str(tmp_path / "cases")
    S.cases_file(path, boundary if name == "boundary" else infix_groups_of_the_unwindowed_fixture())
    for exe in programs:
        out = _run(exe, "cases", path)
        assert re.search(r"cases ok (\d+)", out) and int(re.search(r"cases ok (\d+)", out).group(1)) > 1000, out
