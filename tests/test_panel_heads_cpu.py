"""The 5' heads of the panel search (QUICKED_PANEL_HEADS), the part that needs no GPU: the public surface, what the fixture
holds, the short-sweep equivalence on the definition, the core of quicked_amd/csrc/qe_panel.h -- panel_head_chunk,
panel_member_heads, the tails' walk and keeper behind them and the per-slot bodies: the source k_panel_heads and the kernels
behind it run per lane -- compiled with g++ as a stand-alone program (tests/native/panel_heads_cpu.cpp), plain and under ASan +
UBSan, and the library's host layer against the fake HIP runtime (tests/native/panel_heads_host.cpp), both compared with the
definition (tests/panel_heads_lib.py: the tails of the reversed texts against the reversed members, from the full matrix, in
Python) on the named and random sets of tests/golden/panel_heads_cases.json and on a set made live: both equalities, all three
flag settings, the register forms of 1, 2 and 4 blocks, slices of 1, 2 and K."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_heads_lib as H
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


G = _load("make_panel_heads_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "enum { QUICKED_PANEL_HEADS = 8192 };" in flat
    assert "typedef struct { int32_t pattern, overlap, text_end, score; } quicked_panel_head_t;" in flat
    assert "quicked_batch_configure_panel_heads(quicked_batch_t* batch, int32_t min_overlap);" in flat
    assert "quicked_batch_panel_heads(quicked_batch_t* batch, quicked_panel_head_t* out" in flat
    for phrase in ("Without the bit nothing about any run changes: no launch, no allocation, no copy", "all three bits may be set in one run",      # (the flattening above takes " * " out)
                   "min_overlap <= r <= m - 1", "D^R[r][n] <= floor(r k / m)", "rev() is plain reversal, no complement",
                   "the largest matched length r - D^R[r][n]", "on a tie the smaller score", "then the smaller member index",
                   "text_end is the largest e with ed(member[m-r:m], text[0:e)) == score", "the stretch's start is always 0",
                   "Every field is -1 where no member has a head", "an empty text has none",
                   "the heads of (texts, panel) are the tails of (reversed texts, reversed members) with text_end = n - text_start",
                   "The base mode may be INFIX or PREFIX", "PREFIX together with QUICKED_PANEL_TAILS stays QUICKED_ERROR",
                   "(default 3), independently of the tails' setting", "QUICKED_ERROR outside 1 .. QUICKED_PANEL_MAX_LEN",
                   "QUICKED_ERROR after any run without the bit and after a reload", "QUICKED_ERROR with text_end = -1 where the end pass did not find the head's score",
                   "the bit on quicked_batch_run_panel, _run_panel_scan, _run_search and _run_search_all",
                   "[6] is the block steps of the head sweep, [7] the row steps of its walk", "counters [0] .. [3]",
                   "Not built: heads or tails on quicked_batch_run_panel_scan", "one head per member instead of one per text", "head and tail CIGARs",
                   "reverse-complement members", "queued (sync == 0) panel runs", "128, 256, 1024 and 4096 stay unknown bits"):
        assert phrase in flat, phrase


def test_constants_exports_and_signatures_without_a_device():
    from quicked_amd import capi
    assert capi.PANEL_HEADS == H.HEADS == 8192 and capi.PANEL_TAILS == 2048
    assert {"quicked_batch_configure_panel_heads", "quicked_batch_panel_heads"} <= set(capi.EXPORTS)
    assert callable(capi.ResidentBatch.panel_heads) and callable(capi.ResidentBatch.configure_panel_heads)
    assert capi.PANEL_HEAD_DTYPE.itemsize == 16 and capi.PANEL_HEAD_DTYPE.names == H.HEAD_FIELDS
    lib = capi.lib()
    assert lib.quicked_batch_configure_panel_heads.argtypes == [C.c_void_p, C.c_int32] and lib.quicked_batch_configure_panel_heads.restype == C.c_int
    assert lib.quicked_batch_panel_heads.argtypes == [C.c_void_p, C.c_void_p] and lib.quicked_batch_panel_heads.restype == C.c_int
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    for base in (H.INFIX, H.PREFIX):
        assert lib.quicked_batch_run_panel_all(None, base | capi.PANEL_HEADS, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_configure_panel_heads(None, 3) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_heads(None, None) == capi.QUICKED_ERROR


# ---- the definition and the fixture ---------------------------------------------------------------------------------
def test_the_rule_by_hand():
    a = b"AGATCGGAAGAGC"
    assert H.text_head(b"TCGGAAGAGCCTCTCTCT", [a], [1], 0, 3) == (0, 10, 10, 0)           # the issue's hand case
    assert H.text_head(b"CTCTCTCT", [a], [1], 0, 3) == H.NONE
    assert H.text_head(b"GAGCTTTT", [a], [2], 0, 3) == (0, 4, 4, 0)
    assert H.text_head(b"GAGCTTTT", [a], [2], 0, 5) == H.NONE and H.text_head(b"", [a], [2], 0, 1) == H.NONE
    assert H.text_head(b"GAGCTTTT", [a, a], [2, 2], 0, 3)[0] == 0                          # equal keys: the smaller index
    assert H.text_head(a + b"TTTT", [a], [2], 0, 3)[1] < 13                                # row m is not a head
    assert H.text_head(b"GAAGTGCTTTT", [a], [2], 0, 3) == (0, 7, 7, 1)                     # floor(7 * 2 / 13) = 1: GAAGAGC with one substitution
    assert H.text_head(b"AAGTGCTTTT", [a], [2], 0, 3)[:2] != (0, 6)                        # floor(6 * 2 / 13) = 0
    assert H.text_head(b"TANACCCC", [b"CCTARA"], [0], T.IUPAC, 3) == (0, 4, 4, 0)
    assert H.text_head(b"TANACCCC", [b"CCTARA"], [0], T.IUPAC_PATTERN, 3) == H.NONE
    assert H.text_head(b"GG", [b"TGCA"], [4], 0, 3) == (0, 3, 2, 2)                        # k = m, rows past the text: GCA against GG, the longest stretch
    # the one sentence, on a text with a tail: heads of the mirror
    assert H.text_head(b"CTAGATTTT", [a[::-1]], [2], 0, 3) == (0, 5, 5, 0) and T.text_tail(b"TTTTAGATC", [a], [2], 0, 3) == (0, 5, 4, 0)


def test_the_record_is_the_definition(sets):
    """a fixed sample of the recorded heads, recomputed live (the generator computed every one the same way)"""
    rng = np.random.default_rng(5)
    for name in ("named", "random"):
        for g in sets[name]:
            assert set(g["heads"]) == {(f, mo) for f in G.FLAGS for mo in G.OVERLAPS}
            for (flag, mo), rec in g["heads"].items():
                assert len(rec) == len(g["texts"])
                for i in rng.integers(0, len(g["texts"]), 3):
                    i = int(i)
                    assert rec[i] == H.text_head(g["texts"][i], g["panel"], g["bounds"], flag, mo), (name, g["name"], flag, mo, i)


def test_the_sets_hold_what_they_are_for(sets):
    """the generator asserts the constructions in full; here what can be read off the record"""
    named = {g["name"]: g for g in sets["named"]}
    assert set(named) == {"lengths", "adapters", "whole_bound", "tall", "iupac", "edges", "long"}
    assert os.path.getsize(G.PATH) <= 1000000
    assert [len(q) for q in named["lengths"]["panel"]] == [1, 2, 3, 63, 64, 65, 128, 129, 256]
    assert {len(t) for t in named["lengths"]["texts"]} >= {0, 1, 2, 63, 64, 65, 150}
    assert {t[1] for t in named["lengths"]["heads"][(0, 3)]} >= {63, 64, 65, 127, 128, 129}
    ad = named["adapters"]
    assert ad["heads"][(0, 3)][8][:3] == (0, 15, 15) and ad["heads"][(0, 3)][9][:2] == (0, 20) and ad["heads"][(0, 3)][9][3] == 1
    assert ad["panel"][0] == ad["panel"][3] and ad["heads"][(0, 3)][0][0] == 0 and b"" in ad["texts"]
    assert 0 in ad["bounds"] and any(b >= len(q) for g in sets["named"] for q, b in zip(g["panel"], g["bounds"]))
    assert any(len(t) < hd[1] for t, hd in zip(named["whole_bound"]["texts"], named["whole_bound"]["heads"][(0, 3)]))
    assert any(x != y for x, y in zip(named["iupac"]["heads"][(T.IUPAC, 3)], named["iupac"]["heads"][(T.IUPAC_PATTERN, 3)]))
    ed = named["edges"]
    assert ed["heads"][(0, 3)][0] == (0, 10, 10, 0) and ed["heads"][(0, 3)][1] == H.NONE
    assert {len(t) for t in ed["texts"]} >= {63, 64, 65, 128}
    assert {(len(ed["panel"][h[0]]) - h[1]) for h in ed["heads"][(0, 3)] if h[0] >= 0} >= {1}                  # r = m - 1
    lg = named["long"]
    assert all(300 <= len(t) <= 5000 for t in lg["texts"]) and max(len(t) for t in lg["texts"]) == 5000
    classes = {H.reach(q, b) % 64 for q, b in zip(lg["panel"], lg["bounds"])}
    assert {0, 1, 63} <= classes and len(classes - {0, 1, 63}) >= 1
    assert all(H.reach(q, b) < len(t) for t in lg["texts"] for q, b in zip(lg["panel"], lg["bounds"]))
    # the random set: at least a third of the texts have a head and at least a third have none, under every flag
    for flag in G.FLAGS:
        heads = [t for g in sets["random"] for t in g["heads"][(flag, 3)]]
        have = sum(t[0] >= 0 for t in heads)
        assert 3 * have >= len(heads) and 3 * (len(heads) - have) >= len(heads), (flag, have, len(heads))


def test_the_short_sweep_is_the_full_matrix_answer(sets):
    """member by member: the definition on text[:min(n, m + k)] equals the definition on the whole text, over the fixture"""
    checked = cut = 0
    for name in ("named", "random"):
        for g in sets[name]:
            for text in g["texts"]:
                for q, b in zip(g["panel"], g["bounds"]):
                    c0 = min(len(text), H.reach(q, b))
                    for mo in G.OVERLAPS:
                        assert H.text_head(text[:c0], [q], [b], 0, mo) == H.text_head(text, [q], [b], 0, mo), (name, g["name"], text, q, b, mo)
                    checked += 1
                    cut += c0 < len(text)
    assert checked > 3000 and cut > 1000, (checked, cut)


# ---- the programs ----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the sweep for the host")
    exe = os.path.join(tmp, f"panel_heads_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_heads_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_heads"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def live_groups():
    """a set made now, not recorded: members of every block count, suffixes planted within the row's allowance"""
    rng = np.random.default_rng(78)
    GT = G.GT
    tall = GT.group("live_tall", [GT.rand_seq(rng, m) for m in (100, 130, 200, 256)], [9, 40, 12, 70],
                    [GT.fit(rng, GT.mutate(rng, GT.rand_seq(rng, 1) + GT.rand_seq(rng, int(r)), 2), int(n)) for r, n in zip(rng.integers(1, 250, 30), rng.integers(1, 700, 30))])
    return [G.mirror(GT.random_group(rng, "live", "ACGT", 60, 5)), G.mirror(GT.random_group(rng, "live_letters", "ACGTACGTACGTRYN", 40, 3)), G.mirror(tall)]


@pytest.mark.parametrize("name", ["named", "random", "live"])
def test_sweep_walk_and_keeper_equal_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    H.cases_file(path, live_groups() if name == "live" else sets[name], G.FLAGS, G.OVERLAPS)
    for exe in programs:
        out = _run(exe, "cases", path)
        m = re.search(r"cases ok (\d+) short (\d+) cut (\d+)", out)
        assert m and int(m.group(1)) > 1000 and int(m.group(3)) > 0, out
        if name == "named":
            assert int(m.group(2)) > 0, out            # heads found while the live blocks stopped short of the last block


def test_host_layer_under_address_and_ub_sanitizers(sets, tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    H.cases_file(str(tmp_path / "cases"), sets["named"] + sets["random"], G.FLAGS, G.OVERLAPS)
    exe = build_host("panel_heads_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_heads_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
