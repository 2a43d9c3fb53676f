"""The CIGAR validator (quicked_batch_validate and the in-run check), the part that needs no GPU: the walk, the string parser
and the segment walk of quicked_amd/csrc/qe_check.h -- the source k_check_strings and k_check_segs run per lane and the
host-only build runs in the kernels' place -- compiled with g++ under AddressSanitizer + UBSan and driven over every case the
GPU tests run, plus those no GPU may see untested: run lengths that wrap a 32-bit sum.  Expected verdicts are those of the
restatement in tests/check_lib.py, which is pinned here to the oracle's cigar_check_alignment.

What the same cases find in the walk as it was before qe_check.h (h += cnt, v += cnt and `v + cnt > m` in 32 bits, the
parser admitting every length up to 2^31 - 1), compiled into this driver in the header's place: of the 2 123 cases it fails
367, all of them wraps, and passes the other 1 756.  Built plain with wrapping arithmetic it accepts 111 invalid alignments
(every "wrap back into range" string, "wrap to the end", and the literal and leaf forms of the same sums) and dies of a read
2 GiB off the pair on 141 more ("wrap out of range", "wrap undone later", "length 2147483647I / D first"); the sanitizers
stop it on all 367, the remaining 115 with a signed overflow whose verdict happened to come out right."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import check_lib as L
import oracle_lib as O
from check_lib import M, X, I, D, BIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "quicked_batch.h")


# ---- segment cases: (label, pattern, text, segments) --------------------------------------------------------------------
# a segment = ("L", op, len) | ("R", [(op, len) in alignment order]) | ("B",)
def _flat(segments):
    out = []
    for s in segments:
        if s[0] == "L":
            out.append((s[1], s[2]))
        elif s[0] == "R":
            out += s[1]
        else:
            out.append(None)
    return out


def _lits(runs):
    return [("L", o, n) for o, n in runs]


def _changed(runs, k, how):
    o, n = runs[k]
    return runs[:k] + [((o + 1 + how) % 4, n) if how < 3 else (o, n + (1 if how == 3 else -1))] + runs[k + 1:]


def segment_cases():
    rng = np.random.default_rng(5201)
    c = []
    pairs = [q for q in L.valid_pairs() if len(q[0]) in (0, 1, 9, 17, 23, 64, 65, 130)][::2]
    for p, t, runs in pairs:
        tag = f"m={len(p)}"
        c.append((f"seg {tag} literals only", p, t, _lits(runs)))
        c.append((f"seg {tag} one leaf", p, t, [("R", runs)]))
        c.append((f"seg {tag} no segments", p, t, []))
        c.append((f"seg {tag} empty leaf", p, t, [("R", [])]))
        zl = []
        for o, n in runs:
            zl += [("L", int(rng.integers(0, 4)), 0), ("L", o, n), ("L", int(rng.integers(0, 4)), -3)]
        c.append((f"seg {tag} zero-length and negative literals", p, t, zl))
        for where in ("first", "middle", "last"):
            k = {"first": 0, "middle": len(runs) // 2, "last": len(runs)}[where]
            c.append((f"seg {tag} overflowed leaf {where}", p, t, [("R", runs[:k]), ("B",), ("R", runs[k:])]))
            c.append((f"seg {tag} overflowed leaf {where}, literals", p, t, _lits(runs[:k]) + [("B",)] + _lits(runs[k:])))
        for s in range(len(runs) + 1):
            c.append((f"seg {tag} leaf {s} + literals", p, t, [("R", runs[:s])] + _lits(runs[s:])))
            c.append((f"seg {tag} literals {s} + leaf", p, t, _lits(runs[:s]) + [("R", runs[s:])]))
            if s < len(runs) and runs[s][1] > 1:                        # the border inside run s
                o, n = runs[s]
                k = int(rng.integers(1, n))
                c.append((f"seg {tag} leaf | literal inside run {s}", p, t, [("R", runs[:s] + [(o, k)]), ("L", o, n - k)] + _lits(runs[s + 1:])))
            if runs:
                k = (7 * s + 3) % len(runs)
                for how in range(5):                                     # another operation (3 of them), length + 1, length - 1
                    bad = _changed(runs, k, how)
                    c.append((f"seg {tag} leaf {s} + literals, run {k} changed ({how})", p, t, [("R", bad[:s])] + _lits(bad[s:])))
        # sums that wrap in 32 bits, as literals (any int32 length) and inside a leaf (a run holds up to 2^30 - 1)
        q = 2 ** 30 - 1
        for op in (I, D):
            c.append((f"seg {tag} literal wrap {op} back into range", p, t, [("L", op, BIG), ("L", op, BIG), ("L", op, 2)] + _lits(runs)))
            c.append((f"seg {tag} literal wrap {op} through INT_MIN", p, t, [("L", op, BIG), ("L", op, 1), ("L", op, BIG), ("L", op, 1), ("R", runs)]))
            c.append((f"seg {tag} literal wrap {op} then M", p, t, [("L", op, BIG), ("L", op, 1), ("L", M, 1), ("R", runs)]))
            c.append((f"seg {tag} literal wrap {op} then X", p, t, [("L", op, BIG), ("L", op, 2), ("L", X, 9), ("R", runs)]))
            c.append((f"seg {tag} leaf wrap {op} back into range", p, t, [("R", [(op, q)] * 4 + [(op, 4)] + runs)]))
            c.append((f"seg {tag} leaf wrap {op} then M", p, t, [("R", [(op, q), (op, q), (op, 2), (M, 1)] + runs)]))
        for op in (M, X):
            c.append((f"seg {tag} literal {op} of 2^31 - 1 after the alignment", p, t, [("R", runs), ("L", op, BIG)]))
            c.append((f"seg {tag} literal {op} of 2^31 - 1 after one base", p, t, [("L", M, 1), ("L", op, BIG), ("R", runs)]))
            c.append((f"seg {tag} leaf {op} of 2^30 - 1 twice", p, t, [("R", [(M, 1), (op, q), (op, q), (op, q), (op, q)])]))
    return c


_memo = {}


def all_segment_cases():
    if "seg" not in _memo:
        _memo["seg"] = segment_cases()
    return _memo["seg"]


def _hex(b):
    return b.hex() or "-"


def _write_cases(path, strings, segs):
    lines = [str(len(strings) + len(segs))]
    for _, p, t, s in strings:
        lines.append(f"S {_hex(p)} {_hex(t)} {_hex(s.encode('latin-1'))}")
    for _, p, t, segments in segs:
        lines.append(f"G {_hex(p)} {_hex(t)} {len(segments)}")
        for s in segments:
            if s[0] == "L":
                lines.append(f"L {s[1]} {s[2]}")
            elif s[0] == "B":
                lines.append("B")
            else:
                packed = [(n << 2) | o for o, n in reversed(s[1])]          # back to front, as the traceback leaves them
                assert all(0 <= r < 2 ** 32 for r in packed)
                lines.append(" ".join(["R", str(len(packed))] + [str(r) for r in packed]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the validator for the host")
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "check_cpu.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp, env=None):
    src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "results.txt")
    _write_cases(src, L.cpu_cases(), all_segment_cases())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "check_cpu ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    with open(dst) as f:
        return r, [int(x) for x in f.read().split()]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    """the sanitizer build over every case: (stderr, verdicts)"""
    tmp = str(tmp_path_factory.mktemp("check"))
    exe = _build(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "check_cpu_asan")
    r, got = _run(exe, tmp, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    return r.stderr, got


@pytest.fixture(scope="module")
def expected():
    return ([L.verdict(p, t, s) for _, p, t, s in L.cpu_cases()],
            [L.verdict_ops(p, t, _flat(segments)) for _, p, t, segments in all_segment_cases()])


def test_header_states_the_length_range():
    with open(HEADER) as f:
        text = f.read()
    at = text.index("quicked_status_t quicked_batch_validate")
    doc = text[text.rindex("/*", 0, at):at]
    assert "2147483647" in doc and "at least 1" in doc


def test_restatement_against_the_oracle(expected):
    """check_lib.verdict equals the oracle's cigar_check_alignment on every case the oracle can judge -- none left out --, and
    those are most of the cases, of both verdicts"""
    cases = L.cpu_cases()
    judged = [(k, c) for k, c in enumerate(cases) if L.oracle_can_judge(c[3])]
    bad = [c[0] for k, c in judged if expected[0][k] != int(O.cigar_is_valid(c[1], c[2], c[3]))]
    assert not bad, bad[:5]
    seen = [expected[0][k] for k, _ in judged]
    assert len(judged) > 500 and seen.count(1) > 100 and seen.count(0) > 300, (len(judged), seen.count(1), seen.count(0))
    # the segment cases through the same door: their flattened operations as a string, where every length is positive
    n = 0
    for (label, p, t, segments), want in zip(all_segment_cases(), expected[1]):
        flat = _flat(segments)
        if None in flat or any(ln <= 0 for _, ln in flat):
            continue
        s = L.to_string(flat)
        if L.oracle_can_judge(s):
            n += 1
            assert want == int(O.cigar_is_valid(p, t, s)), label
    assert n > 500, n


def test_mutators_mutate():
    good, mutants = L.count_cases()
    assert all(L.verdict(p, t, s) == 1 for _, p, t, s in good) and len(good) >= 30
    invalid = sum(1 for _, p, t, s in mutants if L.verdict(p, t, s) == 0)
    assert len(mutants) > 300 and invalid >= 0.95 * len(mutants), (invalid, len(mutants))
    kinds = {label.split(" ", 3)[3] for label, *_ in mutants}
    assert len(kinds) == 13, kinds


def test_the_cases_are_what_they_claim():
    """every wrap and limit case is invalid; the wraps "back into range" sum to the start modulo 2^32 with no M or X before"""
    for label, p, t, s in L.wrap_cases_in_range() + L.wrap_cases_out_of_range() + L.length_cases(True) + L.length_cases(False):
        assert L.verdict(p, t, s) == 0, label
    for label, p, t, s in L.wrap_cases_in_range():
        runs, v, h, k = L.parse(s), 0, 0, 0
        while True:                                                      # I and D only until both sums are 0 modulo 2^32 again
            o, n = runs[k]
            assert o in (I, D), label
            v, h, k = (v + (n if o == D else 0)) % 2 ** 32, (h + (n if o == I else 0)) % 2 ** 32, k + 1
            if (v, h) == (0, 0):
                break
        assert any(n == BIG for _, n in runs[:k]) and L.verdict_ops(p, t, runs[k:]) == 1, label
    longs = L.long_string_cases()
    assert all(len(s) == 200000 for _, _, _, s in longs) and [L.verdict(p, t, s) for _, p, t, s in longs] == [1, 0, 1, 0]
    # small pairs (a text is its pattern with up to 10 % more bases); the one exception is the plain 1M1I1D string's pair
    assert all(len(p) <= 300 and len(t) <= 330 for label, p, t, _ in L.gpu_cases() if "66 666 bases" not in label)

def test_walk_against_the_rules_under_the_sanitizers(verdicts, expected):
    err, got = verdicts
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    strings, segs = L.cpu_cases(), all_segment_cases()
    assert len(got) == len(strings) + len(segs)
    want = expected[0] + expected[1]
    labels = [c[0] for c in strings] + [c[0] for c in segs]
    bad = [(labels[k], got[k], want[k]) for k in range(len(got)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5])
    assert len(strings) > 900 and len(segs) > 1000
    # both verdicts in both forms, so an all-ones or all-zeros walk cannot pass
    for part in (got[:len(strings)], got[len(strings):]):
        assert part.count(1) > 100 and part.count(0) > 300, (part.count(1), part.count(0))


def test_plain_build_agrees(verdicts, tmp_path):
    """the walk as the library is built: optimised, no sanitizer"""
    _, got = _run(_build(str(tmp_path), ["-O3"], "check_cpu"), str(tmp_path))
    assert got == verdicts[1]
