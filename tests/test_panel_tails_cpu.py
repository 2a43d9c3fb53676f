"""The 3' tails of the panel search (QUICKED_PANEL_TAILS), the part that needs no GPU: the public surface, what the fixture
holds, the core of quicked_amd/csrc/qe_panel.h -- panel_tail_walk, PanelTailKeeper and the per-slot bodies: the source
k_panel_tails and the kernels behind it run per lane -- compiled with g++ as a stand-alone program
(tests/native/panel_tails_cpu.cpp), plain and under ASan + UBSan, and the library's host layer against the fake HIP runtime
(tests/native/panel_tails_host.cpp, as tests/test_host_panel_cigar.py builds it), both compared with the definition
(tests/panel_tails_lib.py: the full matrix and the rule, in Python) on the named and random sets of
tests/golden/panel_tails_cases.json and on a set made live: both equalities, all three flag settings, the register forms of 1, 2
and 4 blocks, slices of 1, 2 and K."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_tails_lib as T
from native_build import ASAN_UBSAN, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_tails_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "enum { QUICKED_PANEL_TAILS = 2048 };" in flat
    assert "typedef struct { int32_t pattern, overlap, text_start, score; } quicked_panel_tail_t;" in flat
    assert "quicked_batch_configure_panel_tails(quicked_batch_t* batch, int32_t min_overlap);" in flat
    assert "quicked_batch_panel_tails(quicked_batch_t* batch, quicked_panel_tail_t* out" in flat
    for phrase in ("Without the bit nothing about the run changes", "min_overlap <= r <= m - 1", "D[r][n] <= floor(r k / m)",      # (the flattening above takes " * " out)
                   "the largest matched length r - D[r][n]", "on a tie the smaller D[r][n]", "then the smaller member index",
                   "text_start is the smallest s with ed(member[0:r], text[s:n]) == score", "Every field is -1 where no member has a tail",
                   "an empty text has none", "Row m is not a tail", "(default 3)", "QUICKED_ERROR outside 1 .. QUICKED_PANEL_MAX_LEN",
                   "QUICKED_ERROR after any run without the bit and after a reload", "the bit with the base mode QUICKED_SEARCH_PREFIX",
                   "[2] is the row steps of the walk", "Not built: tails on quicked_batch_run_panel_scan", "5' tails",
                   "one tail per member instead of one per text", "tail CIGARs"):
        assert phrase in flat, phrase


def test_constants_exports_and_signatures_without_a_device():
    from quicked_amd import capi
    assert capi.PANEL_TAILS == T.TAILS == 2048
    assert {"quicked_batch_configure_panel_tails", "quicked_batch_panel_tails"} <= set(capi.EXPORTS)
    assert callable(capi.ResidentBatch.panel_tails) and callable(capi.ResidentBatch.configure_panel_tails)
    assert capi.PANEL_TAIL_DTYPE.itemsize == 16 and capi.PANEL_TAIL_DTYPE.names == T.TAIL_FIELDS
    lib = capi.lib()
    assert lib.quicked_batch_configure_panel_tails.argtypes == [C.c_void_p, C.c_int32] and lib.quicked_batch_configure_panel_tails.restype == C.c_int
    assert lib.quicked_batch_panel_tails.argtypes == [C.c_void_p, C.c_void_p] and lib.quicked_batch_panel_tails.restype == C.c_int
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel_all(None, T.INFIX | capi.PANEL_TAILS, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_configure_panel_tails(None, 3) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_tails(None, None) == capi.QUICKED_ERROR


# ---- the definition and the fixture ---------------------------------------------------------------------------------
def test_the_rule_by_hand():
    a = b"AGATCGGAAGAGC"
    assert T.text_tail(b"TTTTAGATC", [a], [2], 0, 3) == (0, 5, 4, 0)
    assert T.text_tail(b"TTTTAGATC", [a], [2], 0, 6) == T.NONE and T.text_tail(b"", [a], [2], 0, 1) == T.NONE
    assert T.text_tail(b"TTTTAGTTCGG", [a], [2], 0, 3) == (0, 7, 4, 1)                 # floor(7 * 2 / 13) = 1
    assert T.text_tail(b"TTTTAGTTCG", [a], [2], 0, 3) == T.NONE                        # floor(6 * 2 / 13) = 0
    assert T.text_tail(b"TTTTAGATC", [a, a], [2, 2], 0, 3)[0] == 0                     # equal keys: the smaller index
    assert T.text_tail(b"TTTTAGATCGGAAGAGC", [a], [2], 0, 3)[1] < 13                   # row m is not a tail
    assert T.text_tail(b"CCCCANAT", [b"ARATCC"], [0], T.IUPAC, 3) == (0, 4, 4, 0)
    assert T.text_tail(b"CCCCANAT", [b"ARATCC"], [0], T.IUPAC_PATTERN, 3) == T.NONE
    assert T.text_tail(b"CCCCANAT", [b"ANATCC"], [0], 0, 3) == (0, 4, 4, 0)            # any two bytes that are not ACGT are equal
    assert T.text_tail(b"GG", [b"ACGT"], [4], 0, 3) == (0, 3, 0, 2)                    # k = m, rows past the text: ACG against GG, the longest stretch
    D = T.matrix(T.equal(b"ACGT", b"TTACG", 0))
    assert D[:, -1].tolist() == [0, 1, 1, 0, 1] and D[3].tolist() == [3, 3, 3, 2, 1, 0]


def test_the_record_is_the_definition(sets):
    """a fixed sample of the recorded tails, recomputed live (the generator computed every one the same way)"""
    rng = np.random.default_rng(5)
    for name in ("named", "random"):
        for g in sets[name]:
            assert set(g["tails"]) == {(f, mo) for f in G.FLAGS for mo in G.OVERLAPS}
            for (flag, mo), rec in g["tails"].items():
                assert len(rec) == len(g["texts"])
                for i in rng.integers(0, len(g["texts"]), 4):
                    i = int(i)
                    assert rec[i] == T.text_tail(g["texts"][i], g["panel"], g["bounds"], flag, mo), (name, g["name"], flag, mo, i)


def test_the_sets_hold_what_they_are_for(sets):
    """the generator asserts the constructions in full; here what can be read off the record"""
    named = {g["name"]: g for g in sets["named"]}
    assert set(named) == {"lengths", "adapters", "whole_bound", "tall", "iupac"}
    assert [len(q) for q in named["lengths"]["panel"]] == [1, 2, 3, 63, 64, 65, 128, 129, 256]
    assert {len(t) for t in named["lengths"]["texts"]} >= {0, 1, 2, 63, 64, 65, 150}
    assert {t[1] for t in named["lengths"]["tails"][(0, 3)]} >= {63, 64, 65, 127, 128, 129}
    ad = named["adapters"]
    assert ad["tails"][(0, 3)][8][:2] == (0, 15) and ad["tails"][(0, 3)][9][:2] == (0, 20) and ad["tails"][(0, 3)][9][3] == 1
    assert ad["panel"][0] == ad["panel"][3] and ad["tails"][(0, 3)][0][0] == 0 and b"" in ad["texts"]
    assert 0 in ad["bounds"] and any(b >= len(q) for g in sets["named"] for q, b in zip(g["panel"], g["bounds"]))
    assert any(len(t) < tl[1] for t, tl in zip(named["whole_bound"]["texts"], named["whole_bound"]["tails"][(0, 3)]))
    assert any(x != y for x, y in zip(named["iupac"]["tails"][(T.IUPAC, 3)], named["iupac"]["tails"][(T.IUPAC_PATTERN, 3)]))
    # the random set: at least a third of the texts have a tail and at least a third have none, under every flag
    for flag in G.FLAGS:
        tails = [t for g in sets["random"] for t in g["tails"][(flag, 3)]]
        have = sum(t[0] >= 0 for t in tails)
        assert 3 * have >= len(tails) and 3 * (len(tails) - have) >= len(tails), (flag, have, len(tails))


# ---- the programs ----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    exe = os.path.join(tmp, f"panel_tails_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_tails_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_tails"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def live_groups():
    """a set made now, not recorded: members of every block count, prefixes planted within the row's allowance"""
    rng = np.random.default_rng(77)
    return [G.random_group(rng, "live", "ACGT", 60, 5), G.random_group(rng, "live_letters", "ACGTACGTACGTRYN", 40, 3),
            G.group("live_tall", [G.rand_seq(rng, m) for m in (100, 130, 200, 256)], [9, 40, 12, 70],
                    [G.fit(rng, G.mutate(rng, G.rand_seq(rng, 1) + G.rand_seq(rng, int(r)), 2), int(n)) for r, n in zip(rng.integers(1, 250, 30), rng.integers(1, 300, 30))])]


@pytest.mark.parametrize("name", ["named", "random", "live"])
def test_walk_and_keeper_equal_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    T.cases_file(path, live_groups() if name == "live" else sets[name], G.FLAGS, G.OVERLAPS)
    for exe in programs:
        out = _run(exe, "cases", path)
        m = re.search(r"cases ok (\d+) short (\d+)", out)
        assert m and int(m.group(1)) > 1000, out
        if name == "named":
            assert int(m.group(2)) > 0, out            # tails found while the live blocks stopped short of the last block


def test_host_layer_under_address_and_ub_sanitizers(sets, tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    T.cases_file(str(tmp_path / "cases"), sets["named"] + sets["random"], G.FLAGS, G.OVERLAPS)
    exe = build_host("panel_tails_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_tails_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
