"""IUPAC degenerate-base search (QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN), the part that needs no GPU: the public
surface, the table and the two plane producers of quicked_amd/csrc/qe_iupac.h, and the recurrence of qe_search.h under the
four-plane equality -- the source k_search<NB, Eq> runs per lane -- compiled with g++ as a stand-alone program
(tests/native/search_iupac_cpu.cpp), plain and under ASan + UBSan, and compared with the brute-force DP of tests/iupac_lib.py
on every case and with edlib + additionalEqualities (tests/golden/search_iupac_cases.json; live where oracle/_ref is built)
wherever edlib judges."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import iupac_lib as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
PREFIX, INFIX = I.PREFIX, I.INFIX
IUPAC, IUPAC_PATTERN = I.IUPAC, I.IUPAC_PATTERN
ALL_LIVE, RULE_WS, RULE_REG = 0, 1, 2
FORMS = (ALL_LIVE, RULE_WS, RULE_REG)
INT_MAX = 2**31 - 1
BOUNDS = (0, 1, 12, "m", INT_MAX)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_search_iupac_cases")
M = G.M


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_documents_the_flags_and_the_argument_rules():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"enum\s*\{\s*QUICKED_SEARCH_IUPAC\s*=\s*16\s*,\s*QUICKED_SEARCH_IUPAC_PATTERN\s*=\s*32\s*\}", text)
    assert re.search(r"QUICKED_SEARCH_PREFIX\s*=\s*1\s*,\s*QUICKED_SEARCH_INFIX\s*=\s*2\s*\}\s*quicked_search_mode_t", text)
    flat = " ".join(text.split())
    for phrase in ("equal when their sets intersect", "mode & 15", "at most one of the two flags", "QUICKED_UNIMPLEMENTED and queues nothing"):
        assert phrase in flat.replace(" * ", " "), phrase


def test_constants_and_refusals_without_a_device():
    from quicked_amd import capi
    assert (capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN) == (16, 32)
    lib = capi.lib()
    assert lib.quicked_batch_run_search(None, INFIX | IUPAC, None, 8, 1, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_run_search_all(None, INFIX | IUPAC, None, 8, 4, 1) == capi.QUICKED_ERROR
    assert os.path.exists(os.path.join(CSRC, "qe_iupac.h"))


def test_the_80_equalities():
    pairs = I.equality_pairs()
    assert len(pairs) == 80 and len(set(pairs)) == 80
    assert ("A", "R") in pairs and ("A", "G") not in pairs and ("R", "Y") not in pairs and ("R", "N") in pairs


# ---- the program -----------------------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the recurrence for the host")
    exe = os.path.join(tmp, f"search_iupac_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "search_iupac_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search_iupac")), [], "plain")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search_iupac_san")), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan")


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _exec(args, ok):
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=ENV)
    assert r.returncode == 0 and ok in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


_RUN = [0]


def run(exe, tmp_path, entries):
    """entries: [(pattern, text, mode, bound, form, flag, cap)] -> per entry a list of int: cap 0 [score, start, end, steps];
    cap > 0 [found, best, stored, steps, (start, end, score) x stored]"""
    _RUN[0] += 1
    d = tmp_path / f"set{_RUN[0]}"
    d.mkdir()
    starts, pp, tp, top_p, top_t = {}, [], [], 0, 0
    poff, toff = np.zeros(len(entries), dtype=np.int64), np.zeros(len(entries), dtype=np.int64)
    for e, ent in enumerate(entries):
        p, t = ent[0], ent[1]
        if (p, t) not in starts:
            starts[(p, t)] = (top_p, top_t)
            pp.append(p); tp.append(t)
            top_p += len(p); top_t += len(t)
        poff[e], toff[e] = starts[(p, t)]
    np.array([len(e[0]) for e in entries], dtype=np.int32).tofile(str(d / "plen.i32"))
    np.array([len(e[1]) for e in entries], dtype=np.int32).tofile(str(d / "tlen.i32"))
    for k, name in ((2, "mode"), (3, "bound"), (4, "form"), (5, "flag"), (6, "cap")):
        np.array([e[k] for e in entries], dtype=np.int32).tofile(str(d / f"{name}.i32"))
    poff.tofile(str(d / "poff.i64")); toff.tofile(str(d / "toff.i64"))
    (d / "ppool.bin").write_bytes(b"".join(pp)); (d / "tpool.bin").write_bytes(b"".join(tp))
    _exec([exe, "search", str(d)], "search ok")
    flat = np.fromfile(str(d / "out.i32"), dtype=np.int32).tolist()
    out, at = [], 0
    for e in entries:
        width = 4 if e[6] == 0 else 4 + 3 * flat[at + 2]
        out.append(flat[at:at + width])
        at += width
    assert at == len(flat)
    return out


def bound_of(b, m):
    return m if b == "m" else b


def check_best(exe, tmp_path, pairs, forms=FORMS, bounds=BOUNDS):
    """every (pair, flag, mode, bound, form) against the brute force"""
    entries, exp = [], []
    for p, t in pairs:
        for flag in (IUPAC, IUPAC_PATTERN):
            for mode in (PREFIX, INFIX):
                a = I.locate(p, t, mode, flag)
                for b in bounds:
                    for form in forms:
                        entries.append((p, t, mode, bound_of(b, len(p)), form, flag, 0))
                        exp.append(I.bounded(a, len(p), bound_of(b, len(p))))
    out = run(exe, tmp_path, entries)
    bad = [(len(e[0]), len(e[1]), e[2:6], out[k][:3], list(exp[k])) for k, e in enumerate(entries) if out[k][:3] != list(exp[k])]
    assert not bad, (len(bad), bad[:8])


def check_edlib(name, pairs):
    """edlib where it judges: equal to the brute force wherever d != m -> (answers judged, of them with d == m)"""
    rec = G.expected(name)
    judged = skipped = 0
    for (p, t), r in zip(pairs, rec):
        for flag in (IUPAC, IUPAC_PATTERN):
            if r is None or not I.edlib_judges(p, t, flag):
                continue
            for mode, e in ((PREFIX, r[0]), (INFIX, r[1])):
                a = I.locate(p, t, mode, flag)
                judged += 1
                assert a[0] == e[0], (len(p), len(t), mode, flag, a, e)
                if a[0] == len(p):
                    skipped += 1
                else:
                    assert list(a) == e, (len(p), len(t), mode, flag, a, e)
    return judged, skipped


def test_table_of_all_256_bytes(plain, sanitized, tmp_path):
    for exe in (plain, sanitized):
        path = str(tmp_path / ("table_" + os.path.basename(exe)))
        _exec([exe, "table", path], "table ok")
        got = np.fromfile(path, dtype=np.uint8).reshape(256, 2)
        assert (got[:, 0] == I.MASK).all(), np.nonzero(got[:, 0] != I.MASK)
        assert (got[:, 1] == I.MASK_ACGT).all(), np.nonzero(got[:, 1] != I.MASK_ACGT)
    assert int(np.count_nonzero(I.MASK)) == 32 and int(np.count_nonzero(I.MASK_ACGT)) == 10


def test_the_two_producers_give_the_same_words(plain, sanitized):
    _exec([plain, "producers"], "producers ok")
    _exec([sanitized, "producers"], "producers ok")


def test_grid_against_brute_force_and_edlib(plain, tmp_path):
    pairs = G.grid_cases()
    assert {(len(p), len(t)) for p, t in pairs} == {(m, n) for m in G.M_LENS for n in G.N_LENS}
    check_best(plain, tmp_path, pairs)
    judged, skipped = check_edlib("grid", pairs)
    print(f"grid: {judged} edlib answers, {skipped} with d == m")
    assert judged >= 2 * len(pairs)


def test_random_against_brute_force_and_edlib(plain, tmp_path):
    pairs = G.random_cases()
    assert len(pairs) == 600
    check_best(plain, tmp_path, pairs)
    judged, skipped = check_edlib("random", pairs)
    jg, sg = check_edlib("grid", G.grid_cases())
    print(f"random: {judged} edlib answers, {skipped} with d == m")
    assert judged >= 2 * len(pairs) and (skipped + sg) * 100 <= judged + jg


def test_named_cases(plain, tmp_path):
    pairs = G.named_cases()
    check_best(plain, tmp_path, pairs)
    check_edlib("named", pairs)
    primer, text = pairs[0]
    assert I.locate(primer, text, INFIX, IUPAC) == (0, 37, 56) and I.locate(primer, text, INFIX, IUPAC_PATTERN) == (0, 37, 56)
    assert [o[1:] for o in I.occurrences(primer, text, INFIX, IUPAC, 0)] == [(56, 0), (133, 0)]      # both concrete variants
    p, t = pairs[1]                                     # an all-N text: every pattern matches it, unless the text is read as ACGT only
    assert I.locate(p, t, INFIX, IUPAC) == (0, 0, len(p)) and I.locate(p, t, INFIX, IUPAC_PATTERN)[0] == len(p)
    p, t = pairs[2]                                     # an all-N pattern matches any ACGT text under both flags
    assert I.locate(p, t, INFIX, IUPAC) == (0, 0, len(p)) == I.locate(p, t, INFIX, IUPAC_PATTERN)
    p, t = pairs[3]
    assert I.locate(p, t, INFIX, IUPAC)[0] == len(p)   # R against Y: disjoint sets
    p, t = pairs[4]
    assert I.locate(p, t, INFIX, IUPAC) == (0, 2, 10)  # U is T
    # the relation is not transitive, and a byte outside the alphabet equals nothing, itself included
    assert I.locate(b"R", b"A", PREFIX, IUPAC)[0] == 0 and I.locate(b"R", b"G", PREFIX, IUPAC)[0] == 0 and I.locate(b"A", b"G", PREFIX, IUPAC)[0] == 1
    assert I.locate(b"-", b"-", PREFIX, IUPAC)[0] == 1 and I.locate(b"X", b"X", INFIX, IUPAC)[0] == 1
    out = run(plain, tmp_path, [(b"AC-GT", b"ttAC-GTtt", INFIX, 5, RULE_REG, IUPAC, 0), (b"acgyn", b"TTACGCGTT", INFIX, 5, RULE_WS, IUPAC_PATTERN, 0),
                                (b"ACGT", b"TTACNTTT", INFIX, 4, RULE_WS, IUPAC, 0), (b"ACGT", b"TTACNTTT", INFIX, 4, RULE_WS, IUPAC_PATTERN, 0)])
    assert [o[:3] for o in out] == [[1, 2, 7], [0, 2, 7], [0, 2, 6], [1, 2, 6]]
    assert [o[:3] for o in out] == [list(I.locate(b"AC-GT", b"ttAC-GTtt", INFIX, IUPAC)), list(I.locate(b"acgyn", b"TTACGCGTT", INFIX, IUPAC_PATTERN)),
                                    list(I.locate(b"ACGT", b"TTACNTTT", INFIX, IUPAC)), list(I.locate(b"ACGT", b"TTACNTTT", INFIX, IUPAC_PATTERN))]


def check_hits(exe, tmp_path, pairs, bounds, caps=(1, 2, 16), forms=FORMS):
    entries, exp = [], []
    for p, t in pairs:
        for flag in (IUPAC, IUPAC_PATTERN):
            for mode in (PREFIX, INFIX):
                for b in bounds:
                    occ = I.occurrences(p, t, mode, flag, b)
                    for cap in caps:
                        for form in forms:
                            entries.append((p, t, mode, b, form, flag, cap))
                            exp.append((occ, cap))
    out = run(exe, tmp_path, entries)
    for k, e in enumerate(entries):
        occ, cap = exp[k]
        got = out[k]
        stored = min(len(occ), cap)
        want = [len(occ), min((o[2] for o in occ), default=-1), stored] + [v for o in occ[:stored] for v in o]
        assert got[:3] + got[4:] == want, (len(e[0]), len(e[1]), e[2:], got, want)
    return entries, out


def test_all_occurrences_on_ties_named_and_random(plain, tmp_path):
    check_hits(plain, tmp_path, G.tie_cases() + G.named_cases(), bounds=(0, 2, 12, INT_MAX))
    pairs = G.random_cases()
    assert len(pairs) == 600
    check_hits(plain, tmp_path, pairs, bounds=(2, 12))
    # the best occurrence is the best search's answer
    for p, t in G.tie_cases()[:20]:
        for flag in (IUPAC, IUPAC_PATTERN):
            occ = I.occurrences(p, t, INFIX, flag, INT_MAX)
            d = min(o[2] for o in occ)
            assert next((o[2], o[0], o[1]) for o in occ if o[2] == d) == I.locate(p, t, INFIX, flag)


def test_acgt_input_gives_the_three_plane_answers_block_steps_included(plain, tmp_path):
    cases = [c for c in M.random_cases() if set(c[0]) | set(c[1]) <= set(b"ACGT")]
    assert len(cases) == 2000                      # every case of that set is ACGT only
    entries = [(p, t, mode, bd, form, flag, 0) for p, t, mode, bd in cases for form in FORMS for flag in (0, IUPAC, IUPAC_PATTERN)]
    out = run(plain, tmp_path, entries)
    for k in range(0, len(entries), 3):
        assert out[k] == out[k + 1] == out[k + 2], (entries[k][2:5], out[k:k + 3])
    lower = [(p.lower(), t, mode, bd) for p, t, mode, bd in cases[:50]] + [(p, t.lower(), mode, bd) for p, t, mode, bd in cases[50:100]]
    entries = [(p, t, mode, bd, RULE_WS, flag, 0) for p, t, mode, bd in lower for flag in (0, IUPAC, IUPAC_PATTERN)]
    out = run(plain, tmp_path, entries)
    for k in range(0, len(entries), 3):
        assert out[k] == out[k + 1] == out[k + 2]
    entries = [(p, t, mode, min(bd, 12), form, flag, 4) for p, t, mode, bd in cases for form in FORMS for flag in (0, IUPAC, IUPAC_PATTERN)]
    out = run(plain, tmp_path, entries)
    for k in range(0, len(entries), 3):
        assert out[k] == out[k + 1] == out[k + 2]


def test_under_address_and_undefined_sanitizers(plain, sanitized, tmp_path):
    """the same program with ASan + UBSan, run on its own, over everything the tests above put through the plain build -- the
    three sets and the ties at the five bounds, the all-occurrences scan, the ACGT cases under all three equalities: no
    report, and the answers of the plain build (which the tests above hold to the brute force)"""
    entries = []
    for p, t in G.grid_cases() + G.named_cases() + G.random_cases() + G.tie_cases():
        for flag in (IUPAC, IUPAC_PATTERN):
            for mode in (PREFIX, INFIX):
                for b in BOUNDS:
                    entries += [(p, t, mode, bound_of(b, len(p)), form, flag, 0) for form in FORMS]
                for bd in (2, 12):
                    entries += [(p, t, mode, bd, form, flag, cap) for form in FORMS for cap in (1, 16)]
    for p, t, mode, bd in M.random_cases():
        entries += [(p, t, mode, bd, form, flag, 0) for form in FORMS for flag in (0, IUPAC, IUPAC_PATTERN)]
        entries += [(p, t, mode, min(bd, 12), RULE_WS, flag, 4) for flag in (0, IUPAC, IUPAC_PATTERN)]
    assert run(sanitized, tmp_path, entries) == run(plain, tmp_path, entries)
