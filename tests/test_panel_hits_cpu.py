"""Panel search, every occurrence (quicked_batch_run_panel_all), the part that needs no GPU: the public surface, the definition
of tests/panel_hits_lib.py, and the core of quicked_amd/csrc/qe_panel.h / qe_search.h -- the generalised SearchHitScan,
panel_text_hits and the count / expand / finish bodies: the source k_panel_hits and its small kernels run per lane -- compiled
with g++ as a stand-alone program (tests/native/panel_hits_cpu.cpp), plain and under ASan + UBSan, and compared with the
definition on every case of tests/golden/panel_hits_cases.json, under both equalities and all three flag settings, with the
member range cut into 1, 2 and K slices and caps of 1, 2 and 4096."""
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
MODES = (PH.PREFIX, PH.INFIX)
FLAGS = (0, PH.IUPAC, PH.IUPAC_PATTERN)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_hits_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_rules():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"int32_t pattern, text_start, text_end, score;\s*\}\s*quicked_panel_occ_t", text)
    flat = " ".join(text.split()).replace(" * ", " ")
    for name in ("quicked_batch_run_panel_all", "quicked_batch_panel_hit_counts", "quicked_batch_panel_hit_total", "quicked_batch_panel_hits"):
        assert name + "(" in flat, name
    for phrase in ("exactly those quicked_batch_run_search_all defines for that pattern against that text with that bound",
                   "ordered by (pattern, text_end), ascending",
                   "stored[i] = min(found[i], max_hits)",
                   "the smallest score among all found occurrences of the text, stored or not",
                   "An empty text keeps QUICKED_EMPTY_SEQUENCE",
                   "the smallest key (score, pattern) among a text's occurrences",
                   "is the QUICKED_PANEL_MATRIX entry [i][p]",
                   "QUICKED_PANEL_MATRIX too: it has no meaning here",
                   "max_hits outside 1 .. 4096", "(non-empty texts) x max_hits above 2^26",
                   "a member longer than QUICKED_PANEL_MAX_LEN bases", "sync == 0", "a batch configured with check != 0",
                   "The three getters below return QUICKED_ERROR (the total: -1) after any run that was not of this kind",
                   "A reload clears the results"):
        assert phrase in flat, phrase


def test_constants_and_refusals_without_a_device():
    from quicked_amd import capi
    assert capi.PANEL_OCC_DTYPE.itemsize == 16 and capi.PANEL_OCC_DTYPE.names == PH.OCC_FIELDS
    lib = capi.lib()
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel_all(None, PH.INFIX, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_hit_counts(None, None, None) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_hit_total(None) == -1
    assert lib.quicked_batch_panel_hits(None, None, None) == capi.QUICKED_ERROR
    for name in ("run_panel_all", "panel_hit_counts", "panel_hits"):
        assert callable(getattr(capi.ResidentBatch, name))


# ---- the definition itself ------------------------------------------------------------------------------------------
def test_expectations_a_reader_can_check():
    panel = [b"ACGTAC", b"TTTT", b"ACGTAC"]
    #         0123456789012345678901
    text = b"GGACGTACGGACGTACCCTTTTT"
    hits = PH.text_hits(text, panel, [0, 0, 0], PH.INFIX, 0)
    # member 0 twice, member 1 once -- TTTTT is a plateau of exact ends 22, 23: the first column counts --, the duplicate last
    assert hits == [(0, 2, 8, 0), (0, 10, 16, 0), (1, 18, 22, 0), (2, 2, 8, 0), (2, 10, 16, 0)]
    assert PH.capped(hits, 2) == (5, [(0, 2, 8, 0), (0, 10, 16, 0)], 0)
    assert PH.capped([], 2) == (0, [], -1)
    assert PH.text_hits(b"", panel, [0, 0, 0], PH.INFIX, 0) == []
    assert PH.best_two(hits) == (0, 0, 2, 8, 1, 0)                 # consequence 1: the best, and the best of the OTHER members
    assert PH.member_best(hits, 3) == ([0, 0, 0], [8, 22, 8])      # consequence 2
    assert PH.text_hits(text, panel, [0, 0, 0], PH.PREFIX, 0) == []
    assert PH.text_hits(b"ACGTACGG", panel, [0, 0, 0], PH.PREFIX, 0) == [(0, 0, 6, 0), (2, 0, 6, 0)]


def test_the_record_is_the_brute_force(sets):
    """a fixed sample of the recorded lists, recomputed live (the generator computed every list the same way)"""
    rng = np.random.default_rng(5)
    for s in sets.values():
        n = len(s["texts"])
        assert set(s["hits"]) == {(m, f, c) for m in MODES for f in FLAGS for c in G.CONFS}
        for (mode, flag, conf), rec in s["hits"].items():
            assert len(rec) == n
            for i in rng.integers(0, n, 4):
                assert rec[int(i)] == PH.text_hits(s["texts"][int(i)], s["panel"], G.bounds_of(s, conf), mode, flag), (mode, flag, conf, int(i))


def test_the_sets_hold_what_they_are_for(sets):
    s = sets["named"]
    assert {len(q) for q in s["panel"]} >= {1, 63, 64, 65, 128, 129, 192, 193, 256}
    assert {len(t) for t in s["texts"]} >= {0, 1, 63, 64, 65, 127, 128, 129, 200}
    assert any(len(t) < len(q) for t in s["texts"] if t for q in s["panel"])
    assert s["panel"][10] == s["panel"][0] and s["panel"][14] == s["panel"][4]
    assert set(b"RYN") <= set(s["panel"][12]) and any(b"N" in t for t in s["texts"])
    uni, own = s["hits"][(PH.INFIX, 0, "uniform")], s["hits"][(PH.INFIX, 0, "own")]
    assert any(sum(1 for o in h if o[0] == 0) >= 2 for h in uni)                       # one member twice
    assert any({0, 13} <= {o[0] for o in h} for h in uni)                              # two different members
    assert any(t and not h for t, h in zip(s["texts"], own))                           # a text with no occurrence
    assert s["uniform"] > min(len(q) for q in s["panel"])                              # the clamp to m is in play
    r = sets["random"]
    assert len(r["texts"]) == 200 and len(r["panel"]) == 12
    uni = r["hits"][(PH.INFIX, 0, "uniform")]
    assert sum(1 for h in uni if any(sum(1 for o in h if o[0] == p) >= 2 for p in range(12))) >= 30
    assert sum(1 for h in uni if len({o[0] for o in h}) >= 2) >= 30
    assert sum(1 for t, h in zip(r["texts"], uni) if t and not h) >= 10
    assert sum(1 for h in uni if len(h) > 2) >= 10


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the panel core for the host")
    exe = os.path.join(tmp, f"panel_hits_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_hits_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_hits"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("name", ["named", "random"])
def test_panel_hits_core_equals_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    PH.cases_file(path, sets[name], MODES, FLAGS)
    for exe in programs:
        out = _run(exe, "cases", path)
        assert re.search(r"cases ok (\d+)", out) and int(re.search(r"cases ok (\d+)", out).group(1)) > 1000, out
