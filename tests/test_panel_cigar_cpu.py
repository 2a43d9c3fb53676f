"""Occurrence alignments (QUICKED_PANEL_CIGARS), the part that needs no GPU: the public surface, what the fixture holds, and the
core of quicked_amd/csrc/qe_panel_align.h -- panel_align_lane / panel_align_occ: the source k_panel_occ_align runs per lane --
compiled with g++ as a stand-alone program (tests/native/panel_cigar_cpu.cpp), plain and under ASan + UBSan, and compared with the
definition (tests/panel_cigar_lib.py: the full matrix and the rule, in Python) on the named and random sets of
tests/golden/panel_cigar_cases.json and on the two sets of tests/golden/panel_hits_cases.json: both equalities, all three flag
settings, styles 0 / 1 / 2, a history that holds every wave and one that holds a single wave, and the checked failure paths (a
score that is off by one, tasks outside the history)."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_cigar_lib as PC
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


GC = _load("make_panel_cigar_cases")
GH = _load("make_panel_hits_cases")
HITS_CAP = 8                     # of the panel_hits sets, whose strings are computed here: a text's first occurrences


@pytest.fixture(scope="module")
def sets():
    return GC.load()


def hits_set(name):
    """a set of tests/golden/panel_hits_cases.json with the definition's strings for every text's first HITS_CAP occurrences under
    the members' own bounds (the program takes whatever occurrences it is handed)"""
    s = dict(GH.load()[name])
    s["hits"] = {k: [h[:HITS_CAP] for h in v] for k, v in s["hits"].items() if k[2] == "own"}
    s["cigars"] = {k: [PC.hit_cigars(t, s["panel"], h, k[1]) for t, h in zip(s["texts"], v)] for k, v in s["hits"].items()}
    return s


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "enum { QUICKED_PANEL_CIGARS = 512 };" in flat
    for phrase in ("Without the bit nothing about either run changes",
                   "quicked_batch_cigars still returns -1 for every pair",
                   "the GLOBAL alignment of its member against text[text_start, text_end)",
                   "D[i][j] == D[i-1][j] + 1 emits D", "D[i][j-1] == D[i-1][j-1] - 1 emits I",
                   "It has exactly `score` edits", "never ends with I",
                   'M means "equal under the run\'s equality"', "R against A is M", "a text N under QUICKED_SEARCH_IUPAC_PATTERN is X",
                   "any two bytes that are not A C G T are equal",
                   "off[j] is never -1 for a stored occurrence of a run that returned QUICKED_OK",
                   "only off and the strings are the contract",
                   "the bit on quicked_batch_run_panel", "the bit together with QUICKED_PANEL_MATRIX",
                   "counter [1] is the block steps of the alignment sweep", "counter [3] the operations emitted",
                   "Not built: alignments for quicked_batch_run_panel and quicked_batch_run_search_all"):
        assert phrase in flat, phrase
    assert "quicked_batch_panel_hit_cigar_bytes(" in flat and "quicked_batch_panel_hit_cigars(" in flat


def test_constants_and_refusals_without_a_device():
    from quicked_amd import capi
    assert capi.PANEL_CIGARS == PC.CIGARS == 512
    assert {"quicked_batch_panel_hit_cigar_bytes", "quicked_batch_panel_hit_cigars"} <= set(capi.EXPORTS)
    assert callable(capi.ResidentBatch.panel_hit_cigars)
    lib = capi.lib()
    pool = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off, ln = np.zeros(1, dtype=np.int64), np.array([4], dtype=np.int32)
    assert lib.quicked_batch_run_panel_all(None, PH.INFIX | capi.PANEL_CIGARS, 1, pool.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 16, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_hit_cigar_bytes(None) == -1
    assert lib.quicked_batch_panel_hit_cigars(None, None, None) == capi.QUICKED_ERROR


# ---- the definition and the fixture ---------------------------------------------------------------------------------
def test_the_rule_by_hand():
    assert PC.cigar(b"ACGT", b"ACGT", 0) == (0, "4M")
    assert PC.cigar(b"AAAA", b"AAA", 0) == (1, "3M1D")                 # the tie: D before I before the diagonal, from the end
    assert PC.cigar(b"ACGT", b"AGT", 0) == (1, "1M1D2M")
    assert PC.cigar(b"AGT", b"ACGT", 0) == (1, "1M1I2M")
    assert PC.cigar(b"ACGT", b"AcNT", 0) == (1, "2M1X1M") and PC.cigar(b"ACNT", b"AC-T", 0) == (0, "4M")
    assert PC.cigar(b"ARGT", b"AAGT", PH.IUPAC) == (0, "4M") and PC.cigar(b"ARGT", b"ACGT", PH.IUPAC) == (1, "1M1X2M")
    assert PC.cigar(b"ACGT", b"ANGT", PH.IUPAC) == (0, "4M") and PC.cigar(b"ACGT", b"ANGT", PH.IUPAC_PATTERN) == (1, "1M1X2M")
    assert [PC.styled("1X3M2I1X1M1D", s) for s in (0, 1, 2)] == ["1X3M2I1X1M1D", "1X3=2I1X1=1D", "1X3M2I2M1D"]


def test_the_record_is_the_definition(sets):
    """a fixed sample of the recorded occurrences and strings, recomputed live (the generator computed every one the same way)"""
    rng = np.random.default_rng(11)
    for name in ("named", "random"):
        s = sets[name]
        assert set(s["hits"]) == set(s["cigars"]) == {(m, f, c) for m in MODES for f in FLAGS for c in GC.SET_CONFS[name]}
        for (mode, flag, conf), rec in s["hits"].items():
            for i in rng.integers(0, len(s["texts"]), 2):
                i = int(i)
                assert rec[i] == PH.text_hits(s["texts"][i], s["panel"], GC.bounds_of(s, conf), mode, flag), (name, mode, flag, conf, i)
                got = s["cigars"][(mode, flag, conf)][i]
                assert got == PC.hit_cigars(s["texts"][i], s["panel"], rec[i], flag), (name, mode, flag, conf, i)
                for o, c in zip(rec[i], got):
                    for style in (0, 1, 2):
                        PC.invariants(PC.styled(c, style), style, len(s["panel"][o[0]]), o[2] - o[1], o[3], mode == PH.PREFIX)


def test_the_named_set_holds_what_it_is_for(sets):
    """the generator asserts the constructions in full; here what can be read off the record"""
    s = sets["named"]
    own, cig = s["hits"][(PH.INFIX, 0, "own")], s["cigars"][(PH.INFIX, 0, "own")]
    every = [(t, o, c) for t, h, cs in zip(s["texts"], own, cig) for o, c in zip(h, cs)]
    assert {len(q) for q in s["panel"]} >= {1, 63, 64, 65, 128, 129, 255, 256}
    assert {o[2] - o[1] for _, o, _ in every} >= {63, 64, 65, 127, 128, 129}
    assert any(o[3] == 0 for _, o, _ in every) and any(o[3] == len(s["panel"][o[0]]) < s["bounds"][o[0]] for _, o, _ in every)
    assert any("5D" in c for _, _, c in every) and any("5I" in c for _, _, c in every)
    assert any(o[1] == 0 and c.startswith("1D") for _, o, c in every) and any(o[2] == len(t) for t, o, _ in every)
    assert max(len(h) for h in own) > 64 and b"" in s["texts"]
    assert any(a != b for a, b in zip(cig, s["cigars"][(PH.INFIX, PH.IUPAC, "own")]))
    assert any(a != b for a, b in zip(s["cigars"][(PH.INFIX, PH.IUPAC, "own")], s["cigars"][(PH.INFIX, PH.IUPAC_PATTERN, "own")]))
    assert any(c.startswith(tuple("%dI" % k for k in range(1, 9))) for cs in s["cigars"][(PH.PREFIX, 0, "own")] for c in cs)      # PREFIX: the top row is counted


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the aligner for the host")
    exe = os.path.join(tmp, f"panel_cigar_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_cigar_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_cigar"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("name", ["named", "random", "hits_named", "hits_random"])
def test_aligner_core_equals_the_definition(programs, sets, tmp_path, name):
    path = str(tmp_path / "cases")
    if name.startswith("hits_"):
        PC.cases_file(path, hits_set(name[5:]), MODES, FLAGS, ("own",))
    else:
        PC.cases_file(path, sets[name], MODES, FLAGS, GC.SET_CONFS[name])
    for exe in programs:
        out = _run(exe, "cases", path)
        assert re.search(r"cases ok (\d+)", out) and int(re.search(r"cases ok (\d+)", out).group(1)) > 1000, out
