"""Approximate pattern search (quicked_batch_run_search), the part that needs no GPU: the public surface, and the recurrence
of quicked_amd/csrc/qe_search.h -- the source k_search<NB> runs per lane -- compiled with g++ as a stand-alone
program (tests/native/search_cpu.cpp), plain and under ASan + UBSan, and compared with the brute-force DP of
tests/search_lib.py on every case and with edlib (tests/golden/search_cases.json; live where oracle/_ref is built) on every
upper-case ACGT case."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import search_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
PREFIX, INFIX = S.PREFIX, S.INFIX
ALL_LIVE, RULE_WS, RULE_REG, LAST_COLUMN = 0, 1, 2, 8
INT_MAX = 2**31 - 1


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_cases", os.path.join(ROOT, "tests", "golden", "make_search_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _cases()
_BF = {}


def brute(p, t, mode):
    key = (p, t, mode)
    if key not in _BF:
        _BF[key] = S.locate(p, t, mode)
    return _BF[key]


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"QUICKED_SEARCH_PREFIX\s*=\s*1\s*,\s*QUICKED_SEARCH_INFIX\s*=\s*2", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_run_search\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*int\s+mode\s*,\s*const\s+int32_t\s*\*", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_locations\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*int32_t\s*\*\s*text_start\s*,\s*int32_t\s*\*\s*text_end", text)


def test_exports_and_prototypes():
    from quicked_amd import capi
    assert {"quicked_batch_run_search", "quicked_batch_locations"} <= set(capi.EXPORTS)
    lib = capi.lib()
    assert hasattr(lib, "quicked_batch_run_search") and hasattr(lib, "quicked_batch_locations")
    assert hasattr(capi.ResidentBatch, "run_search") and hasattr(capi.ResidentBatch, "locations")


def test_null_batch_is_refused():
    from quicked_amd import capi
    lib = capi.lib()
    assert lib.quicked_batch_run_search(None, INFIX, None, 8, 1, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_locations(None, None, None) == capi.QUICKED_ERROR


def test_switch_is_in_the_table():
    with open(os.path.join(CSRC, "qe_pool.h")) as f:
        assert '"QE_SEARCH_FORM"' in f.read()


# ---- the recurrence on the CPU --------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the recurrence for the host")
    exe = os.path.join(tmp, f"search_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "search_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search")), [], "plain")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search_san")), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan")


_RUN = [0]


def run(exe, tmp_path, entries):
    """entries: [(pattern, text, mode, bound, form)] -> (len, 4) int32: score, start, end, block steps"""
    _RUN[0] += 1
    d = tmp_path / f"set{_RUN[0]}"
    d.mkdir()
    starts, pp, tp, top_p, top_t = {}, [], [], 0, 0
    poff, toff = np.zeros(len(entries), dtype=np.int64), np.zeros(len(entries), dtype=np.int64)
    for e, (p, t, _, _, _) in enumerate(entries):
        if (p, t) not in starts:
            starts[(p, t)] = (top_p, top_t)
            pp.append(p); tp.append(t)
            top_p += len(p); top_t += len(t)
        poff[e], toff[e] = starts[(p, t)]
    np.array([len(e[0]) for e in entries], dtype=np.int32).tofile(str(d / "plen.i32"))
    np.array([len(e[1]) for e in entries], dtype=np.int32).tofile(str(d / "tlen.i32"))
    for k, name in ((2, "mode"), (3, "bound"), (4, "form")):
        np.array([e[k] for e in entries], dtype=np.int32).tofile(str(d / f"{name}.i32"))
    poff.tofile(str(d / "poff.i64")); toff.tofile(str(d / "toff.i64"))
    (d / "ppool.bin").write_bytes(b"".join(pp)); (d / "tpool.bin").write_bytes(b"".join(tp))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "search ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = np.fromfile(str(d / "out.i32"), dtype=np.int32).reshape(-1, 4)
    assert len(out) == len(entries)
    return out


def bounds_of(d, m):
    return sorted({0, 1, max(0, d - 1), d, d + 1, 63, 64, m, INT_MAX})


def check(exe, tmp_path, pairs, forms, bounds=None):
    """every (pair, mode, bound, form) against the brute force; -> the outputs by (pair index, mode, bound, form)"""
    entries, exp = [], []
    for i, (p, t) in enumerate(pairs):
        for mode in (PREFIX, INFIX):
            a = brute(p, t, mode)
            for bd in (bounds(i) if bounds else bounds_of(a[0], len(p))):
                for form in forms:
                    entries.append((p, t, mode, bd, form))
                    exp.append(S.bounded(a, len(p), bd))
    out = run(exe, tmp_path, entries)
    bad = [(len(e[0]), len(e[1]), e[2], e[3], e[4], out[k, :3].tolist(), list(exp[k])) for k, e in enumerate(entries)
           if out[k, :3].tolist() != list(exp[k])]
    assert not bad, (len(bad), bad[:8])
    return entries, out


def check_edlib(name, pairs):
    """edlib on a set of upper-case ACGT cases: equal to the brute force wherever d != m (edlib's end location -1), and
    those cases are at most 2 % of the set"""
    rec = M.expected(name)
    skipped = 0
    for (p, t), r in zip(pairs, rec):
        for mode, e in ((PREFIX, r[0]), (INFIX, r[1])):
            a = brute(p, t, mode)
            assert a[0] == e[0], (len(p), len(t), mode, a, e)
            if a[0] == len(p):
                skipped += 1
                continue
            assert list(a) == e, (len(p), len(t), mode, a, e)
    return skipped, 2 * len(pairs)


def test_grid_against_brute_force_and_edlib(plain, tmp_path):
    pairs = M.grid_cases()
    assert {(len(p), len(t)) for p, t in pairs} == {(m, n) for m in M.M_LENS for n in M.N_LENS}
    check(plain, tmp_path, pairs, (ALL_LIVE, RULE_WS, RULE_REG))
    skipped, total = check_edlib("grid", pairs)
    print(f"grid: {total} edlib answers, {skipped} with d == m left to the brute force")
    assert skipped * 50 <= total


def test_ties_smallest_end_longest_stretch(plain, tmp_path):
    pairs = M.tie_cases()
    check(plain, tmp_path, pairs, (ALL_LIVE, RULE_WS, RULE_REG))
    skipped, total = check_edlib("ties", pairs)
    assert skipped * 50 <= total                  # the cap: at most 2 % of a set left to the brute force alone
    # the named no-similarity cases, a set of their own: d == m in both modes, where edlib's end location is -1 and the rule
    # of the header is the definition -- the brute force alone judges them
    none = M.no_similarity_cases()
    check(plain, tmp_path, none, (ALL_LIVE, RULE_WS, RULE_REG))
    assert all(brute(p, t, mode)[0] == len(p) for p, t in none for mode in (PREFIX, INFIX))
    assert [r[0][0] for r in M.expected("no_similarity")] == [len(p) for p, _ in none]
    # what the rules mean, on cases small enough to read
    assert brute(b"CACGT", b"TTGACGT", INFIX) == (1, 2, 7)            # the mismatch G/C keeps the stretch longer than the deletion
    assert brute(b"TTTTT", b"TTTTTTTTTTTT", INFIX) == (0, 0, 5)       # the smallest end of many
    p = pairs[0][0]
    assert brute(p, pairs[0][1], INFIX)[0] == 0 and brute(p, pairs[0][1], INFIX)[2] <= len(pairs[0][1]) - len(p)


def test_live_block_rule_on_long_patterns(plain, tmp_path):
    cases = M.live_cases()
    assert {(len(c[0]), len(c[1])) for c in cases} == set(M.LIVE_SHAPES) and {c[2] for c in cases} == set(M.LIVE_BOUNDS)
    assert len(cases) == 4 * len(M.LIVE_SHAPES) * len(M.LIVE_BOUNDS)          # shape x bound x decoy x indel
    pairs = [(c[0], c[1]) for c in cases]
    # what the cases are for, on the brute force alone: the real occurrence is within its case's bound, it starts at `at`
    # (give or take the edits), and no column before `at` -- the decoy's included -- ends anything within the bound
    for p, t, bound, at in cases:
        d, start, end = brute(p, t, INFIX)
        assert 0 < d <= bound and abs(start - at) <= bound and end > at, (len(p), bound, d, start, end, at)
        assert int(S.last_row(p, t[:at], False)[1:].min()) > bound, (len(p), bound, at)
    decoys = [int(S.last_row(p, t[:at], False)[1:].min()) for p, t, bound, at in cases]
    assert sum(1 for (_, _, bound, _), dd in zip(cases, decoys) if dd <= bound + 6) == len(cases) // 2      # the planted decoys: just beyond
    # every case at its own bound, at the other bound and without one, all blocks live and under the rule
    entries, out = check(plain, tmp_path, pairs, (ALL_LIVE, RULE_WS), bounds=lambda i: M.LIVE_BOUNDS + (len(cases[i][0]),))
    # the rule finds every real occurrence at its case's bound, with the brute force's answer (check() compared them; here:
    # that they were answers, not "beyond")
    found = {(e[0], e[1]) for k, e in enumerate(entries) if e[2] == INFIX and e[4] == RULE_WS and out[k, 0] >= 0
             and e[3] == next(c[2] for c in cases if (c[0], c[1]) == (e[0], e[1]))}
    assert found == set(pairs)
    assert any(out[k, 0] < 0 for k, e in enumerate(entries) if e[2] == INFIX)      # a bound-100 case asked at bound 20
    # the rule computes fewer block steps than the all-live form wherever the bound is far below m, and never more
    steps = {}
    for k, e in enumerate(entries):
        steps.setdefault((e[0], e[1], e[2], e[3]), {})[e[4]] = int(out[k, 3])
    assert all(v[RULE_WS] <= v[ALL_LIVE] for v in steps.values())
    # (along an occurrence or a decoy the live region grows by a block per chunk -- a triangle, half the blocks on average
    # over its m columns; elsewhere a bound of 20 keeps the rows below ~83 / 0.5 = 170 alive, 3 blocks of 16 or 47: less than
    # half of the all-live work in total)
    ratios = {(len(key[0]), len(key[1]), key[2]): round(v[ALL_LIVE] / v[RULE_WS], 2) for key, v in steps.items() if key[3] == 20}
    print(ratios)
    assert all(2 * v[RULE_WS] < v[ALL_LIVE] for key, v in steps.items() if key[3] == 20 and key[2] == INFIX)
    skipped, _ = check_edlib("live", pairs)
    assert skipped == 0


def test_random_shapes_and_bounds(plain, tmp_path):
    cases = M.random_cases()
    assert len(cases) == 2000
    entries = [(p, t, mode, bd, form) for p, t, mode, bd in cases for form in (ALL_LIVE, RULE_WS, RULE_REG)]
    out = run(plain, tmp_path, entries)
    bad = []
    for k, e in enumerate(entries):
        exp = S.bounded(brute(e[0], e[1], e[2]), len(e[0]), e[3])
        if out[k, :3].tolist() != list(exp):
            bad.append((len(e[0]), len(e[1]), e[2], e[3], e[4], out[k, :3].tolist(), exp))
    assert not bad, (len(bad), bad[:8])
    rec = M.expected("random")
    skipped = 0
    for (p, t, mode, _), r in zip(cases, rec):
        a, e = brute(p, t, mode), r[0 if mode == PREFIX else 1]
        assert a[0] == e[0]
        if a[0] == len(p):
            skipped += 1
        else:
            assert list(a) == e, (len(p), len(t), mode, a, e)
    print(f"random: {skipped} of {len(cases)} with d == m")
    assert skipped * 50 <= len(cases)


def test_symbols_n_lower_case_iupac(plain, tmp_path):
    check(plain, tmp_path, M.symbol_cases(), (ALL_LIVE, RULE_WS, RULE_REG))
    # case folded, every non-ACGT byte one symbol
    out = run(plain, tmp_path, [(b"ACGTN", b"ttacgtRtt", INFIX, 5, RULE_REG), (b"ACGTN", b"ttacgtAtt", INFIX, 5, RULE_WS)])
    assert out[0, :3].tolist() == [0, 2, 7] and out[1, 0] == 1


def test_prefix_read_at_the_last_column_is_the_global_distance(plain, tmp_path):
    pairs = [(p, t) for p, t in M.grid_cases()[::5]] + [(c[0], c[1]) for c in M.live_cases()[:2]]
    entries = [(p, t, PREFIX, INT_MAX, form | LAST_COLUMN) for p, t in pairs for form in (ALL_LIVE, RULE_WS, RULE_REG)]
    out = run(plain, tmp_path, entries)
    for k, (p, t, _, _, _) in enumerate(entries):
        g = int(S.last_row(p, t, True)[-1])
        assert out[k, :3].tolist() == ([g, -1, len(t)] if g <= len(p) else [-1, -1, -1]), (len(p), len(t), out[k].tolist(), g)


def test_under_address_and_undefined_sanitizers(plain, sanitized, tmp_path):
    """the same program with ASan + UBSan over the grid, the ties, the symbols and the long patterns: no report, and the
    answers of the plain build"""
    entries = []
    for p, t in M.grid_cases() + M.tie_cases() + M.no_similarity_cases() + M.symbol_cases():
        for mode in (PREFIX, INFIX):
            for bd in (0, 3, 64, INT_MAX):
                entries += [(p, t, mode, bd, form) for form in (ALL_LIVE, RULE_WS, RULE_REG)]
    for p, t, bound, _ in M.live_cases():
        entries += [(p, t, mode, bound, form) for mode in (PREFIX, INFIX) for form in (ALL_LIVE, RULE_WS)]
    assert (run(sanitized, tmp_path, entries) == run(plain, tmp_path, entries)).all()
