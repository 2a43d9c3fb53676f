"""The fixed cases of the IUPAC search tests (tests/test_search_iupac_cpu.py, tests/test_gpu_search_iupac.py) and the recorder
of edlib's answers to them.

As make_search_cases.py: the sequences are regenerated from seeds by the functions below, which the tests import; only
edlib's ANSWERS are recorded, in tests/golden/search_iupac_cases.json: per case [d, start, end] for SHW (prefix) and HW
(infix) with EDLIB_TASK_LOC and additionalEqualities = the 80 pairs of distinct IUPAC letters whose sets intersect
(tests/iupac_lib.py), end = endLocations[0] + 1.  Every case but the named one with U is upper-case over the 15 letters (that
one is recorded as null), so the record is edlib's opinion on QUICKED_SEARCH_IUPAC for all of them, and on
QUICKED_SEARCH_IUPAC_PATTERN for those whose text is ACGT only.
Where oracle/_ref is built the tests ask edlib live and require its answers to equal this record.  The brute-force DP of
tests/iupac_lib.py -- the definition -- is always computed live; the recorder requires edlib to equal it on every case it
records (on d alone where d == m: edlib's end location is -1 there), and such cases to be at most 1 % of grid + random.

    python tests/golden/make_search_iupac_cases.py        # needs oracle/_ref (make -C oracle ref)
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

_spec = importlib.util.spec_from_file_location("make_search_cases", os.path.join(HERE, "make_search_cases.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FIXTURE = os.path.join(HERE, "search_iupac_cases.json")
SEED = 20261019
PREFIX, INFIX = 1, 2
M_LENS, N_LENS, RATES = M.M_LENS, M.N_LENS, M.RATES
ALPHABETS = (list(b"ACGTN"), list(b"ACGTRYKMN"), list(b"ACGTRYSWKMBDHVN"), list(b"ACGTACGTACGTRYN"))      # the last: mostly concrete
# the letters that contain a base, for turning a concrete pattern base into a degenerate one
CONTAINING = {b: [l for l, s in (("R", "AG"), ("Y", "CT"), ("S", "CG"), ("W", "AT"), ("K", "GT"), ("M", "AC"), ("B", "CGT"), ("D", "AGT"),
                                 ("H", "ACT"), ("V", "ACG"), ("N", "ACGT")) if chr(b) in s] for b in b"ACGT"}


def grid_cases():
    """[(pattern, text)]: every (m, n) of M_LENS x N_LENS with the occurrence planted at the start, at the end and across a
    column-64 boundary; the alphabet rotates through ALPHABETS, the planted edit rate through RATES"""
    rng = np.random.default_rng(SEED)
    out, v = [], 0
    for m in M_LENS:
        for n in N_LENS:
            for where in (0, 1, 2):
                alphabet = ALPHABETS[v % len(ALPHABETS)]
                pattern = bytes(M._rand(rng, m, alphabet))
                out.append((pattern, M.plant(rng, pattern, n, where, RATES[v % len(RATES)], alphabet)))
                v += 1
    return out


def random_cases(count=600):
    """[(pattern, text)]: m in 1 .. 199, n in m .. m + 199, the alphabets, the three places and the rates in rotation"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for i in range(count):
        alphabet = ALPHABETS[i % len(ALPHABETS)]
        m = int(rng.integers(1, 200))
        n = int(rng.integers(m, m + 200))
        p = bytes(M._rand(rng, m, alphabet))
        out.append((p, M.plant(rng, p, n, i % 3, RATES[i % len(RATES)], alphabet)))
    return out


def degenerate(rng, pattern, every):
    """`pattern` (ACGT) with about one base in `every` replaced by an IUPAC letter that contains it"""
    q = bytearray(pattern)
    for i in range(len(q)):
        if int(rng.integers(0, every)) == 0:
            c = CONTAINING[q[i]]
            q[i] = ord(c[int(rng.integers(0, len(c)))])
    return bytes(q)


def tie_cases():
    """the tie cases of make_search_cases.py (two occurrences of equal cost, stretches that may start with an edit), each as
    it is and with a fifth of its pattern bases made degenerate"""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for p, t in M.tie_cases():
        out.append((p, t))
        out.append((degenerate(rng, p, 5), t))
    return out


PRIMER = b"GTGYCAGCMGCCGCGGTAA"


def named_cases():
    rng = np.random.default_rng(SEED + 3)
    f = [bytes(M._rand(rng, k)) for k in (37, 58, 41)]
    p20 = bytes(M._rand(rng, 20))
    return [(PRIMER, f[0] + b"GTGTCAGCCGCCGCGGTAA" + f[1] + b"GTGCCAGCAGCCGCGGTAA" + f[2]),      # both concrete variants of the primer
            (p20, b"N" * 50),                                                                   # an all-N text
            (b"N" * 20, bytes(M._rand(rng, 50))),                                               # an all-N pattern
            (b"R" * 10, b"Y" * 30),                                                             # disjoint sets: d = m
            (b"ACGUUGCA", b"TTACGTTGCATT")]                                                     # U is T


SETS = {"grid": grid_cases, "random": random_cases, "ties": tie_cases, "named": named_cases}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def expected(name):
    """edlib's [[d, start, end] for SHW, [..] for HW] per case of a set: live where oracle/_ref is built (and then equal to
    the record), else the record"""
    import iupac_lib as I
    import search_lib as S
    rec = load()[name]
    pairs = SETS[name]()
    assert len(rec) == len(pairs), f"{FIXTURE}[{name}] is stale: regenerate it"
    if not S.have_edlib():
        return rec
    live = [[I.edlib_locate(p, t, PREFIX), I.edlib_locate(p, t, INFIX)] if I.edlib_judges(p, t, I.IUPAC) else None for p, t in pairs]
    assert live == rec, f"{FIXTURE}[{name}] differs from the live oracle: regenerate it"
    return live


def main():
    import iupac_lib as I
    import search_lib as S
    assert S.have_edlib(), "build oracle/_ref first (make -C oracle ref)"
    out = {"seed": SEED}
    skipped = {}
    for name, make in SETS.items():
        rec = []
        skipped[name] = 0
        for p, t in make():
            if not I.edlib_judges(p, t, I.IUPAC):          # (U: not one of the 15 letters; the brute force alone judges it)
                assert name == "named"
                rec.append(None)
                continue
            r = [I.edlib_locate(p, t, PREFIX), I.edlib_locate(p, t, INFIX)]
            for mode, e in ((PREFIX, r[0]), (INFIX, r[1])):
                a = I.locate(p, t, mode, I.IUPAC)
                assert a[0] == e[0], (name, len(p), len(t), mode, a, e)
                if a[0] == len(p):
                    skipped[name] += 1
                else:
                    assert list(a) == e, (name, len(p), len(t), mode, a, e)
            rec.append(r)
        out[name] = rec
        print(name, len(rec), "cases,", skipped[name], "answers with d == m")
    total = 2 * (len(out["grid"]) + len(out["random"]))
    assert (skipped["grid"] + skipped["random"]) * 100 <= total, (skipped, total)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
