"""Every occurrence within the bound (quicked_batch_run_search_all), the part that needs no GPU: the public surface, and the
recurrence of quicked_amd/csrc/qe_search.h -- the source k_search_hits<NB> runs per lane -- compiled with g++ as a stand-alone
program (tests/native/search_hits_cpu.cpp), plain and under ASan + UBSan, and compared with the brute force of
tests/search_hits_lib.py on every case, with the best search's brute force (search_lib.locate) for the smallest occurrence,
and with edlib's location lists (tests/golden/search_hits_cases.json; live where oracle/_ref is built) for the occurrences of
the best score on every upper-case ACGT case."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import search_hits_lib as H
import search_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
PREFIX, INFIX = S.PREFIX, S.INFIX
MODES = (PREFIX, INFIX)
ALL_LIVE, RULE_WS, RULE_REG = 0, 1, 2
FORMS = (ALL_LIVE, RULE_WS, RULE_REG)
CAPS = (1, 2, 4096)


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_hits_cases", os.path.join(ROOT, "tests", "golden", "make_search_hits_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _cases()
_BEST = {}


def best_search(p, t, mode):
    key = (p, t, mode)
    if key not in _BEST:
        _BEST[key] = S.locate(p, t, mode)
    return _BEST[key]


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+text_start\s*,\s*text_end\s*,\s*score\s*;\s*\}\s*quicked_hit_t\s*;", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_run_search_all\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*int\s+mode\s*,\s*const\s+int32_t\s*\*\s*max_dist\s*,"
                     r"\s*int32_t\s+max_dist_all\s*,\s*int32_t\s+max_hits\s*,\s*int\s+sync\s*\)", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_hit_counts\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*int32_t\s*\*\s*found\s*,\s*int32_t\s*\*\s*stored\s*\)", text)
    assert re.search(r"int64_t\s+quicked_batch_hit_total\s*\(\s*quicked_batch_t\s*\*\s*batch\s*\)", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_hits\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*quicked_hit_t\s*\*\s*hits\s*,\s*int64_t\s*\*\s*hit_off", text)


def test_exports_prototypes_and_null_batch():
    from quicked_amd import capi
    names = {"quicked_batch_run_search_all", "quicked_batch_hit_counts", "quicked_batch_hit_total", "quicked_batch_hits"}
    assert names <= set(capi.EXPORTS)
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(capi.ResidentBatch, "run_search_all") and hasattr(capi.ResidentBatch, "hits")
    assert capi.HIT_DTYPE.itemsize == 12 and capi.HIT_DTYPE.names == ("text_start", "text_end", "score")
    assert lib.quicked_batch_run_search_all(None, INFIX, None, 8, 4, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_hit_counts(None, None, None) == capi.QUICKED_ERROR
    assert lib.quicked_batch_hit_total(None) == -1
    assert lib.quicked_batch_hits(None, None, None) == capi.QUICKED_ERROR


# ---- the recurrence on the CPU --------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the recurrence for the host")
    exe = os.path.join(tmp, f"search_hits_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "search_hits_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search_hits")), [], "plain")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("search_hits_san")), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan")


_RUN = [0]


def run(exe, tmp_path, entries):
    """entries: [(pattern, text, mode, bound, form, cap)] -> [(found, best, steps, [(start, end, score)])]"""
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
    for k, name in ((2, "mode"), (3, "bound"), (4, "form"), (5, "cap")):
        np.array([e[k] for e in entries], dtype=np.int32).tofile(str(d / f"{name}.i32"))
    poff.tofile(str(d / "poff.i64")); toff.tofile(str(d / "toff.i64"))
    (d / "ppool.bin").write_bytes(b"".join(pp)); (d / "tpool.bin").write_bytes(b"".join(tp))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "search hits ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    raw = np.fromfile(str(d / "out.i32"), dtype=np.int32).tolist()
    out, at = [], 0
    for _ in entries:
        found, best, stored, steps = raw[at:at + 4]
        at += 4
        out.append((found, best, steps, [tuple(raw[at + 3 * h:at + 3 * h + 3]) for h in range(stored)]))
        at += 3 * stored
    assert at == len(raw)
    return out


def cycled_bound(i, d, m):
    return (0, 1, max(0, d - 1), d, d + 1, 63, 64, m)[i % 8]


def check_set(exe, tmp_path, pairs, bounds=None, forms=FORMS):
    """every (pair, mode, bound, form, cap) against the brute force; the four required properties -> {(pair, mode, bound, form): steps}"""
    entries, keys = [], []
    for i, (p, t) in enumerate(pairs):
        for mode in MODES:
            d = best_search(p, t, mode)[0]
            for bd in (bounds(i) if bounds else (cycled_bound(i, d, len(p)),)):
                for form in forms:
                    for cap in CAPS:
                        entries.append((p, t, mode, bd, form, cap))
                        keys.append((i, mode, bd, form, cap))
    out = run(exe, tmp_path, entries)
    got = dict(zip(keys, out))
    bad, steps = [], {}
    for (i, mode, bd, form, cap), (found, best, st, hits) in got.items():
        p, t = pairs[i]
        exp = H.occurrences(p, t, mode, bd)
        # equal to the brute force; found whatever the cap; the stored ones are the first by text_end
        if found != len(exp) or hits != exp[:cap] or best != (min(o[2] for o in exp) if exp else -1):
            bad.append((i, len(p), len(t), mode, bd, form, cap, found, hits[:4], exp[:4]))
        steps[(i, mode, bd, form)] = st
        if cap == CAPS[-1]:
            # the smallest occurrence is the best search's answer for the same bound, d == m included
            want = S.bounded(best_search(p, t, mode), len(p), bd)
            if H.best_of(hits) != tuple(want):
                bad.append(("best", i, len(p), len(t), mode, bd, form, H.best_of(hits), want))
            for small in CAPS[:-1]:
                other = got[(i, mode, bd, form, small)]
                if other[0] != found or other[3] != hits[:small]:
                    bad.append(("cap", i, mode, bd, form, small, other[0], found))
    assert not bad, (len(bad), bad[:6])
    return steps


def check_edlib(name, pairs):
    """the occurrences of score d without a bound: their ends are edlib's end list with every member whose predecessor is in the
    list removed, their starts edlib's starts of those ends; the brute force live equals the record; -> (left to the brute force, all)"""
    rec = G.load()[name]
    assert len(rec) == len(pairs), f"{G.FIXTURE}[{name}] is stale: regenerate it"
    skipped = 0
    for (p, t), r in zip(pairs, rec):
        for col, mode in enumerate(MODES):
            occ = H.occurrences(p, t, mode, len(p))
            assert [list(o) for o in occ] == r[col], (name, len(p), len(t), mode)
            e = r[2 + col]
            if S.have_edlib():
                live = H.edlib_best_occurrences(p, t, mode)
                assert (None if live is None else [live[0], live[1]]) == e, f"{G.FIXTURE}[{name}] differs from the live oracle: regenerate it"
            d = min(o[2] for o in occ)
            assert d == best_search(p, t, mode)[0]
            if e is None:
                assert d == len(p)
                skipped += 1
                continue
            assert e[0] == d
            assert [[o[0], o[1]] for o in occ if o[2] == d] == e[1], (name, len(p), len(t), mode, occ[:4], e)
    return skipped, 2 * len(pairs)


@pytest.mark.parametrize("name", ["grid", "ties", "random"])
def test_existing_sets_against_brute_force_and_edlib(name, plain, tmp_path):
    pairs = G.SETS[name]()
    check_set(plain, tmp_path, pairs)
    skipped, total = check_edlib(name, pairs)
    print(f"{name}: {total} edlib answers, {skipped} left to the brute force")
    assert skipped * 50 <= total


def test_the_three_sets_are_the_1360_cases_with_many_occurrences():
    pairs = [q for name in ("grid", "ties", "random") for q in G.SETS[name]()]
    assert 2 * len(pairs) == 1360
    many = sum(1 for p, t in pairs for mode in MODES if len(H.occurrences(p, t, mode, len(p))) > 1)
    print(f"{many} of 1360 cases have more than one occurrence at bound m")
    assert many * 3 >= 1360


@pytest.mark.parametrize("name", ["borders", "edges", "short", "tandem", "adjacent", "lengths"])
def test_shapes_of_the_scan(name, plain, tmp_path):
    pairs = G.SETS[name]()
    check_set(plain, tmp_path, pairs)
    check_set(plain, tmp_path, pairs, bounds=lambda i: (len(pairs[i][0]), 3))
    skipped, total = check_edlib(name, pairs)
    assert skipped * 50 <= total
    rows = [(p, t, H.row_of(p, t, INFIX)) for p, t in pairs]
    if name == "borders":
        # what the cases are for: a valley whose plateau starts at or before a chunk's last column and ends behind it
        for p, t, row in rows:
            ok = False
            for _, e, v in H.occurrences(p, t, INFIX, len(p)):
                last = e
                while last < len(t) and row[last] == v:
                    last += 1
                ok = ok or any(e <= b < last for b in (64, 128))
            assert ok, (len(p), len(t))
    if name == "edges":
        assert any(H.occurrences(p, t, INFIX, len(p))[0][1] == 1 for p, t, _ in rows)
        assert sum(1 for p, t, row in rows if H.occurrences(p, t, INFIX, len(p))[-1][2] == row[-1]) >= 10      # pending at the last column
    if name == "short":
        assert all(len(t) < len(p) for p, t in pairs)
    if name == "tandem":
        assert all(len(p) == 16 and len(t) == 1000 and len(H.occurrences(p, t, INFIX, 3)) >= 24 for p, t in pairs)
    if name == "adjacent":
        for p, t in pairs:
            ends = [e for _, e, v in H.occurrences(p, t, INFIX, len(p) // 8)]
            assert len(ends) >= 2 and min(b - a for a, b in zip(ends, ends[1:])) < 2 * len(p)
    if name == "lengths":
        assert {len(p) for p, _ in pairs} == {1, 63, 64, 65, 256, 257, 300}


def test_dead_blocks_between_occurrences(plain, tmp_path):
    pairs = G.SETS["dead"]()
    bd = G.DEAD_BOUND
    for p, t in pairs:
        occ = H.occurrences(p, t, INFIX, bd)
        assert len(p) == 1000 and len(occ) == 2 and occ[1][1] - occ[0][1] >= 1500, [(len(p), o) for o in occ]
        # the decoy: a valley just beyond the bound
        assert any(bd < v <= bd + 6 for _, _, v in H.occurrences(p, t, INFIX, bd + 6))
    steps = check_set(plain, tmp_path, pairs, bounds=lambda i: (bd, 1000), forms=(ALL_LIVE, RULE_WS))
    # the lower blocks died between the copies: along each of the three copies the live region grows by a block per chunk
    # (a triangle, half of the 16 blocks over its 1 000 columns), elsewhere bound 20 keeps three blocks alive -- about half
    # of the all-live work; a sweep whose blocks stayed alive after the first copy would compute over 80 % of it
    for i in range(len(pairs)):
        assert 3 * steps[(i, INFIX, bd, RULE_WS)] < 2 * steps[(i, INFIX, bd, ALL_LIVE)]
    skipped, _ = check_edlib("dead", pairs)
    assert skipped == 0


def test_symbols_n_lower_case_iupac(plain, tmp_path):
    pairs = G.SETS["symbols"]()
    check_set(plain, tmp_path, pairs)
    check_set(plain, tmp_path, pairs, bounds=lambda i: (len(pairs[i][0]),))
    rec = G.load()["symbols"]
    for (p, t), r in zip(pairs, rec):
        assert [[list(o) for o in H.occurrences(p, t, mode, len(p))] for mode in MODES] == r[:2] and r[2:] == [None, None]
    out = run(plain, tmp_path, [(b"ACGTN", b"ttacgtRttACGTYa", INFIX, 0, RULE_REG, 8), (b"ACGTN", b"ttacgtAtt", INFIX, 1, RULE_WS, 8)])
    assert out[0][0] == 2 and out[0][3] == [(2, 7, 0), (9, 14, 0)] and out[1][1] == 1


def test_under_address_and_undefined_sanitizers(plain, sanitized, tmp_path):
    """the same program with ASan + UBSan over every set: no report, no write past a sink, and the answers of the plain build"""
    entries = []
    for name, make in G.SETS.items():
        pairs = make()
        if name == "random":
            pairs = pairs[::4]
        for i, (p, t) in enumerate(pairs):
            for mode in MODES:
                bds = (G.DEAD_BOUND, 1000) if name == "dead" else (cycled_bound(i, best_search(p, t, mode)[0], len(p)), len(p))
                entries += [(p, t, mode, bd, form, cap) for bd in bds for form in FORMS for cap in CAPS]
    assert run(sanitized, tmp_path, entries) == run(plain, tmp_path, entries)
