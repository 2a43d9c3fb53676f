"""Alignment tags (quicked_batch_configure_tags), the part that needs no GPU: the public surface, and the walker of
quicked_amd/csrc/qe_tags.h -- the source k_tags_segs runs per lane and the host-only build runs in the kernels' place --
compiled with g++ and driven over segment lists against the restatement of the definitions in tests/tags_lib.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tags_lib as T
from tags_lib import M, X, I, D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "quicked_batch.h")
CALLS = ["quicked_batch_configure_tags", "quicked_batch_pair_stats", "quicked_batch_md_bytes", "quicked_batch_md"]


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_enum():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"quicked_status_t\s+quicked_batch_configure_tags\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*int\s+tags\s*\)", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_pair_stats\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*quicked_pair_stats_t\s*\*", text)
    assert re.search(r"int64_t\s+quicked_batch_md_bytes\s*\(\s*quicked_batch_t\s*\*", text)
    assert re.search(r"quicked_status_t\s+quicked_batch_md\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*char\s*\*\s*md_pool\s*,\s*int64_t\s*\*", text)
    assert re.search(r"QUICKED_TAG_STATS\s*=\s*1\s*,\s*QUICKED_TAG_MD\s*=\s*2\s*,\s*QUICKED_TAG_NO_CIGAR\s*=\s*4", text)
    assert "NM is the score" in text and "PATTERN is SAM's reference" in text


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_struct_is_32_bytes_in_c_and_cpp(lang, tmp_path):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.fail("gcc / g++ are needed to compile the header")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    check = "_Static_assert" if lang == "c" else "static_assert"
    src.write_text('#include <stddef.h>\n#include "quicked_batch.h"\n'
                   f'{check}(sizeof(quicked_pair_stats_t) == 32, "32 bytes");\n'
                   f'{check}(offsetof(quicked_pair_stats_t, longest_match) == 24 && offsetof(quicked_pair_stats_t, columns) == 28, "layout");\n'
                   f'{check}((QUICKED_TAG_STATS | QUICKED_TAG_MD | QUICKED_TAG_NO_CIGAR) == 7, "bits");\n'
                   "int main(void) { return 0; }\n")
    subprocess.run([cc, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)


def test_exports_and_binding():
    from quicked_amd import capi
    lib = capi.lib()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
    for name in ("configure_tags", "pair_stats", "md"):
        assert hasattr(capi.ResidentBatch, name)
    assert (capi.TAG_STATS, capi.TAG_MD, capi.TAG_NO_CIGAR) == (1, 2, 4)


def test_switch_is_in_the_table():
    with open(os.path.join(CSRC, "qe_pool.h")) as f:
        assert '"QE_TAGS_WAVE"' in f.read()


def test_null_batch_is_refused():
    from quicked_amd import capi
    lib = capi.lib()
    assert lib.quicked_batch_configure_tags(None, 1) == capi.QUICKED_ERROR
    out = np.zeros(8, dtype=np.int32)
    off = np.zeros(1, dtype=np.int64)
    assert lib.quicked_batch_pair_stats(None, out.ctypes.data) == capi.QUICKED_ERROR
    assert lib.quicked_batch_md(None, None, off.ctypes.data) == capi.QUICKED_ERROR
    assert lib.quicked_batch_md_bytes(None) == 0


# ---- the walker on the CPU ------------------------------------------------------------------------------------------
# A case = (pattern bytes, segments); a segment = ("L", op, len) | ("R", [(op, len) in alignment order]) | ("B",)
def _ops(segments):
    out = []
    for s in segments:
        if s[0] == "L":
            out.append((s[1], s[2]))
        elif s[0] == "R":
            out += s[1]
    return out


def _consumes(ops):
    return sum(n for o, n in ops if o != I and n > 0)


def _pattern(rng, m, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), m).tolist()) if m else b""


def _case(rng, segments, alphabet=b"ACGT"):
    return (_pattern(rng, _consumes(_ops(segments)), alphabet), segments)


def _split(rng, ops):
    """one operation sequence cut into segments at random places -- inside runs too, so equal neighbours meet at the
    borders --, as leaves, literals and zero-length literals"""
    pieces = []
    for o, n in ops:
        while n > 0:
            k = int(rng.integers(1, n + 1)) if rng.random() < 0.4 else n
            pieces.append((o, k))
            n -= k
    segs, cur = [], []
    for pc in pieces:
        r = rng.random()
        if r < 0.25:
            if cur:
                segs.append(("R", cur)); cur = []
            segs.append(("L", pc[0], pc[1]))
            if rng.random() < 0.3:
                segs.append(("L", int(rng.integers(0, 4)), 0))
        else:
            # inside a leaf neighbouring runs differ (the traceback merges): a piece equal to the last one opens a new leaf
            if cur and (cur[-1][0] == pc[0] or r < 0.4):
                segs.append(("R", cur)); cur = []
            cur.append(pc)
    if cur:
        segs.append(("R", cur))
    if rng.random() < 0.2:
        segs.append(("R", []))
    return segs


def _random_ops(rng, nruns, weights, maxlen):
    ops, last = [], -1
    for _ in range(nruns):
        o = int(rng.choice(4, p=weights))
        if o == last:
            o = (o + 1 + int(rng.integers(0, 3))) % 4
        ops.append((o, int(rng.integers(1, maxlen + 1))))
        last = o
    return ops


def hand_made(rng):
    c = []
    # the known answers of the issue
    c.append((b"ACGT", [("R", [(M, 1), (X, 1), (M, 2)])]))
    c.append((b"ACGTACGT", [("L", M, 2), ("R", [(D, 2)]), ("R", [(D, 3)]), ("L", M, 1)]))
    # borders inside D, I, M and X runs; zero-length literals in between
    for op in (M, X, I, D):
        c.append(_case(rng, [("R", [(M, 3), (op, 2)]), ("L", op, 0), ("R", [(op, 3), (M, 4) if op != M else (X, 1)])]))
        c.append(_case(rng, [("L", op, 2), ("L", I, 0), ("L", op, 5), ("R", [(op, 1)])]))
    # D I D; leading and trailing indels
    c.append((b"ACGT", [("R", [(D, 2), (I, 3), (D, 2)])]))
    c.append(_case(rng, [("R", [(I, 2), (M, 5), (D, 3)])]))
    c.append(_case(rng, [("R", [(D, 4), (M, 5), (I, 1)])]))
    c.append(_case(rng, [("R", [(D, 1), (X, 1), (D, 1), (X, 2), (I, 1), (X, 1)])]))
    # pattern length 1 (and 0: insertions only)
    c += [(b"A", [("L", M, 1)]), (b"C", [("L", X, 1)]), (b"G", [("R", [(I, 3), (D, 1)])]), (b"", [("L", I, 4)])]
    # digit counts: match runs of 9 / 10 / 99 / 100 / 1000+, before a mismatch, before a deletion and at the end
    for n in (9, 10, 99, 100, 999, 1000, 1001, 12345):
        c.append(_case(rng, [("R", [(M, n), (X, 1), (M, n), (D, 2), (M, n)])]))
        c.append(_case(rng, [("R", [(M, n - 4)]), ("L", M, 4), ("L", X, 1)]))
    # raw bytes: lower case, IUPAC, bytes above 127
    c.append(_case(rng, [("R", [(M, 2), (X, 3), (D, 4), (M, 1)])], alphabet=b"acgtNRY\x80\xfe"))
    # a leaf whose run buffer overflowed
    c.append((b"ACGT", [("R", [(M, 2)]), ("B",), ("L", M, 2)]))
    return c


def adversarial(rng):
    """the sequences that press on the MD bound: all X, D and I alternating, 1M1X alternating"""
    c = []
    for m in (1, 2, 9, 10, 11, 100, 1000):
        c.append(_case(rng, [("R", [(X, m)])]))
        for unit in ([(D, 1), (I, 1)], [(I, 1), (D, 1)], [(M, 1), (X, 1)], [(D, 2), (I, 1)], [(M, 9), (D, 1), (I, 1)]):
            c.append(_case(rng, [("R", unit * m)]))
    return c


def random_cases(rng, count):
    c = []
    for q in range(count):
        w = [(0.4, 0.2, 0.2, 0.2), (0.25, 0.25, 0.25, 0.25), (0.1, 0.3, 0.2, 0.4)][q % 3]
        ops = _random_ops(rng, int(rng.integers(1, 40)), w, [3, 12, 150][q % 3])
        c.append(_case(rng, _split(rng, ops), alphabet=b"ACGT" if q % 5 else b"ACGTacgtN"))
    return c


_memo = {}


def all_cases():
    if not _memo:
        rng = np.random.default_rng(20260)
        _memo["cases"] = hand_made(rng) + adversarial(rng) + random_cases(rng, 3000)
    return _memo["cases"]


def _write_cases(path, cases):
    lines = [str(len(cases))]
    for pattern, segments in cases:
        lines.append(f"{pattern.hex() or '-'} {len(segments)}")
        for s in segments:
            if s[0] == "L":
                lines.append(f"L {s[1]} {s[2]}")
            elif s[0] == "B":
                lines.append("B")
            else:
                packed = [(n << 2) | o for o, n in reversed(s[1])]          # back to front, as the traceback leaves them
                lines.append(" ".join(["R", str(len(packed))] + [str(r) for r in packed]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _read_results(path):
    out = []
    with open(path) as f:
        for line in f:
            w = line.split()
            out.append((int(w[0]), tuple(int(x) for x in w[1:9]), int(w[9]), b"" if w[10] == "-" else bytes.fromhex(w[10])))
    return out


def _expected(case):
    pattern, segments = case
    if any(s[0] == "B" for s in segments):
        return (0, T.NONE_STATS, 0, b"")
    ops = _ops(segments)
    want = T.md(ops, pattern)
    return (1, T.stats(ops), len(want), want)


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walker for the host")
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "tags_cpu.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp, cases, env=None):
    src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "results.txt")
    _write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "tags_cpu ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r, _read_results(dst)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tags"))
    _, got = _run(_build(tmp, [], "tags_cpu"), tmp, all_cases())
    return got


def test_known_answers(results):
    cases = all_cases()
    assert cases[0][0] == b"ACGT" and results[0] == (1, (3, 1, 0, 0, 0, 0, 2, 4), 3, b"1C2")
    assert cases[1][0] == b"ACGTACGT" and results[1][3] == b"2^GTACG1" and results[1][1][5] == 1 and results[1][1][3] == 5
    did = next(k for k, c in enumerate(cases) if c[1] == [("R", [(D, 2), (I, 3), (D, 2)])])
    assert results[did][3] == b"0^AC0^GT0" and results[did][1] == (0, 0, 3, 4, 1, 2, 0, 7)


def test_walker_against_the_definitions(results):
    cases = all_cases()
    assert len(results) == len(cases) > 3000
    bad = [(k, results[k], _expected(c)) for k, c in enumerate(cases) if results[k] != _expected(c)]
    assert not bad, bad[:3]
    # the set has what it is meant to have: borders inside runs of every operation, four-digit numbers, no-alignment cases
    assert any(re.search(rb"\d{5}", r[3]) for r in results) and any(r[0] == 0 for r in results)
    def border_inside(case, op):          # two neighbouring segments meet inside a run of `op`
        ends = [(_ops([s])[0][0], _ops([s])[-1][0]) for s in case[1] if _ops([s])]
        return any(a[1] == op == b[0] for a, b in zip(ends, ends[1:]))
    for op in (M, X, I, D):
        assert any(border_inside(c, op) for c in cases), op


def test_md_bound_holds(results):
    """no string of the set -- the adversarial sequences among them -- needs more than 3 m + 11 bytes with its terminator,
    and the sequences that press on it come close: D and I alternating take three characters per pattern base"""
    cases = all_cases()
    worst = 0.0
    for (pattern, _), r in zip(cases, results):
        assert r[2] + 1 <= T.md_bound(len(pattern)), (len(pattern), r[2])
        if len(pattern) >= 100:
            worst = max(worst, r[2] / len(pattern))
    assert 2.9 < worst <= 3.01, worst


def test_under_address_and_undefined_sanitizers(results, tmp_path):
    exe = _build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tags_cpu_asan")
    r, got = _run(exe, str(tmp_path), all_cases(),
                  env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert got == results
