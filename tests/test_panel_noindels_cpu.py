"""The mismatch-only panel runs (QUICKED_PANEL_NO_INDELS), the part that needs no GPU: the public surface, what the fixture holds
and that it is the definition's, and the core of quicked_amd/csrc/qe_panel_ham.h -- the sweep, the keeper form, the scalar
valley scan and the finish bodies: the source k_panel_ham and k_panel_ham_hits run per lane -- compiled with g++ as a stand-alone
program (tests/native/panel_noindels_cpu.cpp), plain and under ASan + UBSan, and compared with the definition
(tests/panel_noindels_lib.py: plain loops over bytes) on tests/golden/panel_noindels_cases.json and on a seeded random set made
live: both equalities, all three flag settings, the register forms of 1, 2 and 4 blocks, slices of 1, 2 and K, caps of 1, 2
and 4096."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import panel_lib as PL
import panel_noindels_lib as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_noindels_cases")


@pytest.fixture(scope="module")
def groups():
    return G.load()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "enum { QUICKED_PANEL_NO_INDELS = 32768 };" in flat
    for phrase in ("Without the bit nothing about any run changes: no launch, no allocation, no copy",
                   "H[s] = #{ r in [0, m) : member[r] and text[s + r] are NOT equal under the run's equality }",
                   "INFIX E = {m, .., n}, PREFIX E = {m}, n < m: E is empty", "Every column outside E counts as higher than every value",
                   "text_start = text_end - m always", "no start pass is launched", "R[e] <= k, R[e] < R[e - 1]",
                   "Every QUICKED_ERROR rule of the two runs comes first, unchanged",
                   "QUICKED_PANEL_CIGARS, QUICKED_PANEL_TAILS or QUICKED_PANEL_HEADS beside it", "sync == 0, also on a batch object that quicked_batch_configure_panel_queue switched on",
                   "a member over QUICKED_PANEL_MAX_LEN; check != 0", "the bit on quicked_batch_run_panel_scan, _run_search and _run_search_all",
                   "[1] .. [7] are 0", "kernel_times slot [0] holds the launches",
                   "Not built: CIGARs, tails and heads under the bit; queued flagged runs; the windowed run under the bit"):
        assert phrase in flat, phrase


def test_the_binding_names_the_bit():
    from quicked_amd import capi
    assert capi.PANEL_NO_INDELS == N.NO_INDELS == 32768
    for other in (capi.PANEL_MATRIX, capi.PANEL_CIGARS, capi.PANEL_TAILS, capi.PANEL_HEADS, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN, 15):
        assert not capi.PANEL_NO_INDELS & other


# ---- the definition and its record ----------------------------------------------------------------------------------
def test_the_hand_cases():
    """worked by hand from the contract"""
    R = N.R_of(b"ACGT", b"AACGTACGAACCT", N.INFIX, 0)
    assert R == {4: 3, 5: 0, 6: 4, 7: 4, 8: 4, 9: 1, 10: 4, 11: 4, 12: 3, 13: 1}
    assert N.best_of(R, 4) == (0, 5) and N.best_of(R, 0) == (0, 5) and N.best_of({4: 3}, 2) == (-1, -1)
    assert N.valleys_of(R, 1) == [(5, 0), (9, 1), (13, 1)]            # 13: a plateau of one column that reaches the end
    assert N.valleys_of(R, 4) == [(5, 0), (9, 1), (13, 1)]            # 4 and 12 are no valleys: the first other value after them is lower
    assert N.R_of(b"ACGT", b"AACGTACG", N.PREFIX, 0) == {4: 3} and N.R_of(b"ACGT", b"ACG", N.INFIX, 0) == {}
    assert N.valleys_of({5: 2, 6: 2, 7: 2}, 2) == [(5, 2)]            # a plateau counts once, at its first end
    assert N.valleys_of({5: 1, 6: 1, 7: 0}, 2) == [(7, 0)]            # ... and not at all when the row falls behind it
    # the three equalities
    assert not N.differ(ord("a"), ord("A"), 0) and not N.differ(ord("N"), ord("x"), 0) and N.differ(ord("N"), ord("A"), 0)
    assert not N.differ(ord("R"), ord("g"), N.IUPAC) and N.differ(ord("R"), ord("C"), N.IUPAC) and not N.differ(ord("N"), ord("N"), N.IUPAC)
    assert N.differ(ord("N"), ord("N"), N.IUPAC_PATTERN) and not N.differ(ord("N"), ord("u"), N.IUPAC_PATTERN) and N.differ(ord("X"), ord("X"), N.IUPAC)
    # an indel and a shift: within one edit, three mismatches away
    member, text = b"ACGTTGCAAGGC", b"TTACGTGCAAGGCTT"
    assert PL.pair_answer(member, text, N.INFIX, 0)[0] == 1 and min(N.H_of(member, text, 0)) >= 3


def test_the_record_is_the_definition(groups):
    """a fixed sample of the recorded results, recomputed live (the generator computed every one the same way)"""
    rng = np.random.default_rng(11)
    for g in groups.values():
        assert set(g["results"]) == {(m, f) for m in G.MODES for f in G.FLAGS}
        for (mode, flag), r in g["results"].items():
            assert len(r["d"]) == len(r["e"]) == len(r["found"]) == len(r["occ"]) == len(g["texts"])
            for i in rng.integers(0, len(g["texts"]), 2):
                i = int(i)
                D, E = N.matrix([g["texts"][i]], g["panel"], g["bounds"], mode, flag)
                hits = N.text_hits(g["texts"][i], g["panel"], g["bounds"], mode, flag)
                assert (r["d"][i], r["e"][i], r["found"][i], r["occ"][i]) == (D[0], E[0], len(hits), hits[:G.CAP]), (g["name"], mode, flag, i)
                assert N.member_best(hits, len(g["panel"])) == (D[0], E[0])                       # consequence 2, on the definition
                assert N.best_two(hits) == N.reduce_text(D[0], E[0], g["panel"])                   # consequence 1


def test_the_sets_hold_what_they_are_for(groups):
    assert set(groups) == {"lengths", "homopolymer", "indels", "single", "bytes", "panel130", "wave65"}
    assert os.path.getsize(G.PATH) <= 1000000
    assert {g["set"] for g in groups.values()} == {"named", "shape"}
    assert [len(q) for q in groups["lengths"]["panel"]] == [1, 2, 24, 63, 64, 65, 128, 129, 255, 256]
    lg = groups["lengths"]
    for m in (len(q) for q in lg["panel"]):
        assert {len(t) - m + 1 for t in lg["texts"]} >= {0, 1, 2, 63, 64, 65, 129}, m
    assert b"" in lg["texts"] and {len(t) for t in lg["texts"]} >= {128, 129, 192, 193}
    for g in groups.values():
        assert all(b >= 0 for b in g["bounds"])
    bounds = {(b if b < N.INT32_MAX else "max") if b != len(q) else "m" for g in groups.values() for q, b in zip(g["panel"], g["bounds"])}
    assert bounds >= {0, 1, "m", "max"}
    assert sorted({len(g["panel"]) for g in groups.values()}) == [1, 5, 10, 130]
    assert len(groups["wave65"]["texts"]) == 65 and len({len(t) for t in groups["wave65"]["texts"][:64]}) >= 6
    p130 = groups["panel130"]["panel"]
    assert p130[7] == p130[3] and p130[66] == p130[64]
    hp = groups["homopolymer"]
    assert all(len(set(q)) == 1 for q in hp["panel"]) and max(hp["results"][(N.INFIX, 0)]["found"]) > 2
    assert any(set(t) & set(b"acgtn") for t in groups["bytes"]["texts"]) and b"N" * 16 in groups["bytes"]["texts"]
    assert any(set(q) & set(b"RYN") for q in groups["bytes"]["panel"])
    # a kernel that ran the edit-distance sweep could not pass: a third of every set's entries differ from that run's
    for name in ("named", "shape"):
        differ = total = 0
        for g in groups.values():
            if g["set"] != name:
                continue
            D, E = PL.cut(*PL.matrix(g["texts"], g["panel"], N.INFIX, 0), g["panel"], g["bounds"])
            r = g["results"][(N.INFIX, 0)]
            for i in range(len(g["texts"])):
                for p in range(len(g["panel"])):
                    differ += (int(D[i][p]), int(E[i][p])) != (r["d"][i][p], r["e"][i][p])
                    total += 1
        assert 3 * differ >= total, (name, differ, total)
    # the planted indels: within one edit, beyond under this definition
    g = groups["indels"]
    D, _ = PL.cut(*PL.matrix(g["texts"][:12], g["panel"], N.INFIX, 0), g["panel"], g["bounds"])
    assert ((D >= 0) & (D <= 1)).all() and all(d == -1 for row in g["results"][(N.INFIX, 0)]["d"][:12] for d in row)


def test_the_numpy_form_is_the_plain_loops(groups):
    for name in ("lengths", "bytes", "wave65"):
        g = groups[name]
        texts = [t for t in g["texts"] if t]
        for flag in G.FLAGS:
            for q in g["panel"][:6]:
                got = N.H_batch(q, texts, flag)
                for i, t in enumerate(texts):
                    want = N.H_of(q, t, flag)
                    assert got[i, :len(want)].tolist() == want and (got[i, len(want):] == -1).all(), (name, flag, i)


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the sweep for the host")
    exe = os.path.join(tmp, f"panel_noindels_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_noindels_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("panel_noindels"))
    return [_build(tmp, [], "plain"), _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "san")]


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def live_groups():
    """a seeded random set made now, not recorded: members of every block count, a third of the texts with a planted member"""
    rng = np.random.default_rng(4242)
    out = []
    for name, lens, alphabet in (("live_short", (5, 17, 24, 31, 40), "ACGT"), ("live_tall", (64, 65, 100, 128, 190, 256), "ACGT"), ("live_letters", (8, 20, 70), "ACGTACGTACGTRYNacgt")):
        panel = [G.rand_seq(rng, m, alphabet) for m in lens]
        bounds = [int(rng.integers(0, 6)) if p % 3 else N.INT32_MAX for p in range(len(panel))]
        texts = []
        for i in range(24):
            n = int(rng.integers(1, 3 * max(lens) // 2 + 40))
            t = G.rand_seq(rng, n, alphabet)
            if i % 3 == 0:
                q = G.substitute(rng, panel[int(rng.integers(0, len(panel)))], int(rng.integers(0, 4))) if alphabet == "ACGT" else panel[int(rng.integers(0, len(panel)))]
                t = G.plant(rng, max(n, len(q) + 3), q)
            texts.append(t)
        out.append({"name": name, "panel": panel, "bounds": bounds, "texts": texts, "results": N.results_of(texts, panel, bounds, G.CAP)})
    return out


@pytest.mark.parametrize("name", ["fixture", "live"])
def test_sweep_keeper_and_valley_scan_equal_the_definition(programs, groups, tmp_path, name):
    path = str(tmp_path / "cases")
    N.cases_file(path, live_groups() if name == "live" else list(groups.values()), G.CAP)
    for exe in programs:
        out = _run(exe, "cases", path)
        m = re.search(r"cases ok (\d+) occ (\d+)", out)
        assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000, out
