"""Panel search (quicked_batch_run_panel), the part that needs no GPU: the public surface, and the core of
quicked_amd/csrc/qe_panel.h -- the keeper, panel_text and panel_start_task: the source k_search_panel and k_panel_reduce run
per lane -- compiled with g++ as a stand-alone program (tests/native/search_panel_cpu.cpp), plain and under ASan + UBSan, and
compared with the definition of tests/panel_lib.py (the per-pair brute forces and the key order) on every case of
tests/golden/search_panel_cases.json, under both equalities and all three flag settings, with the member range cut into 1, 2
and K slices."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_lib as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
MODES = (P.PREFIX, P.INFIX)
FLAGS = (0, P.IUPAC, P.IUPAC_PATTERN)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_search_panel_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_rules():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"enum\s*\{\s*QUICKED_PANEL_MAX_PATTERNS\s*=\s*4096\s*,\s*QUICKED_PANEL_MAX_LEN\s*=\s*256\s*\}", text)
    assert re.search(r"enum\s*\{\s*QUICKED_PANEL_MATRIX\s*=\s*64\s*\}", text)
    assert re.search(r"int32_t pattern, score, text_start, text_end, second_pattern, second_score;\s*\}\s*quicked_panel_hit_t", text)
    flat = " ".join(text.split()).replace(" * ", " ")
    for phrase in ("the batch's own patterns are ignored and may all be empty",
                   "ordered by the key (score, panel index), ascending",
                   "a duplicate of the best, at a higher index, is the runner-up with the same score",
                   "-1 is reported where there is none",
                   "computed for the best member only",
                   "QUICKED_EMPTY_SEQUENCE is reported for an empty text only",
                   "Without the flag the matrix getter returns QUICKED_ERROR",
                   "panel members are the \"pattern\" side",
                   "a NULL batch", "a base mode that is not PREFIX or INFIX", "both IUPAC flags, or an unknown bit",
                   "a batch configured with check != 0",
                   "n_patterns outside 1 .. QUICKED_PANEL_MAX_PATTERNS",
                   "a member of length 0", "a negative bound", "n_patterns above 2^28",
                   "a member longer than QUICKED_PANEL_MAX_LEN bases", "sync == 0",
                   "The two panel getters return QUICKED_ERROR after any run that was not a panel run"):
        assert phrase in flat, phrase


def test_constants_and_refusals_without_a_device():
    from quicked_amd import capi
    assert (capi.PANEL_MATRIX, capi.PANEL_MAX_PATTERNS, capi.PANEL_MAX_LEN) == (64, 4096, 256)
    assert capi.PANEL_HIT_DTYPE.itemsize == 24 and capi.PANEL_HIT_DTYPE.names == P.HIT_FIELDS
    lib = capi.lib()
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel(None, P.INFIX, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_results(None, None) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_matrix(None, None, None) == capi.QUICKED_ERROR
    assert os.path.exists(os.path.join(CSRC, "qe_panel.h"))


# ---- the definition itself ------------------------------------------------------------------------------------------
def test_expectations_a_reader_can_check():
    from quicked_amd import capi
    assert capi.PANEL_HIT_DTYPE.names == P.HIT_FIELDS              # the order of the fields below is the structure's
    panel = [b"ACGTAC", b"ACGTAC", b"ACGAAC", b"TTTTTTTT"]
    texts = [b"GGACGTACGG", b"", b"GGACGAACGG", b"CCCC"]
    hits, D, E = P.expected(texts, panel, [1, 1, 1, 1], P.INFIX, 0)
    assert hits[0].tolist() == [0, 0, 2, 8, 1, 0]                 # the duplicate at the higher index is the runner-up
    assert hits[1].tolist() == [-1] * 6 and D[1].tolist() == [-1] * 4
    assert hits[2].tolist() == [2, 0, 2, 8, 0, 1]
    assert hits[3].tolist() == [-1] * 6                            # nothing within 1
    assert D[0].tolist() == [0, 0, 1, -1] and E[0].tolist() == [8, 8, 8, -1]
    hits, _, _ = P.expected(texts, panel, [1, 1, 1, 1], P.PREFIX, 0)
    assert hits[0].tolist() == [-1] * 6                            # two bases in front: distance 2 from the text's start


def test_the_record_is_the_brute_force(sets):
    """a fixed sample of the recorded matrices, recomputed live (the generator computed every entry the same way)"""
    rng = np.random.default_rng(5)
    for s in sets.values():
        n, k = len(s["texts"]), len(s["panel"])
        assert set(s["matrix"]) == {(m, f) for m in MODES for f in FLAGS}
        for (mode, flag), (D, E) in s["matrix"].items():
            assert D.shape == (n, k) and E.shape == (n, k)
            for _ in range(25):
                i, p = int(rng.integers(0, n)), int(rng.integers(0, k))
                want = P.pair_answer(s["panel"][p], s["texts"][i], mode, flag) if s["texts"][i] else (-1, -1)
                assert (int(D[i, p]), int(E[i, p])) == want, (mode, flag, i, p)


def test_the_members_at_once_equal_the_pairs_one_by_one(sets):
    s = sets["named"]
    for mode in MODES:
        for flag in FLAGS:
            for i in (0, 5, 9, 16, 23, 31, 33, 36):
                d, e = P.text_answers(s["texts"][i], s["panel"], mode, flag)
                assert [(int(a), int(b)) for a, b in zip(d, e)] == [P.pair_answer(q, s["texts"][i], mode, flag) for q in s["panel"]]


def test_the_sets_hold_what_they_are_for(sets):
    s = sets["named"]
    assert {len(q) for q in s["panel"]} >= {1, 24, 63, 64, 65, 128, 129, 192, 193, 256}
    assert {len(t) for t in s["texts"]} >= {0, 1, 63, 64, 65, 127, 128, 129, 300}
    assert s["panel"][10] == s["panel"][0] and sum(a != b for a, b in zip(s["panel"][0], s["panel"][11])) == 1
    assert set(b"RYN") <= set(s["panel"][12]) and any(b"N" in t for t in s["texts"])
    r = sets["random"]
    assert len(r["texts"]) == 200 and len(r["panel"]) == 12
    hits, _, _ = P.expected(r["texts"], r["panel"], [r["uniform"]] * 12, P.INFIX, 0, *r["matrix"][(P.INFIX, 0)])
    assert int((hits[:, 4] >= 0).sum()) >= 50
    assert int(((hits[:, 4] >= 0) & (hits[:, 5] == hits[:, 1])).sum()) >= 10
    assert sum(1 for i, t in enumerate(r["texts"]) if t and hits[i, 0] < 0) >= 10
    for s in sets.values():                                        # the bounds cycle over 0, 1, d - 1, d, d + 1, m, INT32_MAX
        for p, q in enumerate(s["panel"]):
            if p % 7 in (0, 1):
                assert s["bounds"][p] == p % 7
            if p % 7 == 5:
                assert s["bounds"][p] == len(q)
            if p % 7 == 6:
                assert s["bounds"][p] == P.INT32_MAX


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the panel core for the host")
    exe = os.path.join(tmp, f"search_panel_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "search_panel_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("search_panel"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_keeper_takes_like_a_sort_and_merges_in_any_grouping(programs):
    for exe in programs:
        assert "keeper ok" in _run(exe, "keeper")


def test_four_block_store_has_zero_planes_for_absent_blocks(programs):
    for exe in programs:
        assert "blocks ok" in _run(exe, "blocks")


@pytest.mark.parametrize("name", ["named", "random"])
def test_panel_core_equals_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    P.cases_file(path, sets[name], MODES, FLAGS)
    for exe in programs:
        out = _run(exe, "cases", path)
        assert re.search(r"cases ok (\d+)", out) and int(re.search(r"cases ok (\d+)", out).group(1)) > 1000, out
