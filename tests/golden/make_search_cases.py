"""The fixed cases of the pattern-search tests (tests/test_search_cpu.py, tests/test_gpu_search.py) and the recorder of
edlib's answers to them.

The sequences are regenerated from seeds by the functions below, which the tests import; only edlib's ANSWERS are recorded,
in tests/golden/search_cases.json: per upper-case ACGT case [d, start, end] for SHW (prefix) and HW (infix) with
EDLIB_TASK_LOC, end = endLocations[0] + 1.  Where oracle/_ref is built the tests ask edlib live and require its answers to
equal this record; where it is not, the record alone.  The brute-force DP of tests/search_lib.py -- the definition -- is
always computed live, for every case.

    python tests/golden/make_search_cases.py        # needs oracle/_ref (make -C oracle ref)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "search_cases.json")
SEED = 20261018
PREFIX, INFIX = 1, 2
M_LENS = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 300)
N_LENS = (1, 63, 64, 65, 128, 130, 1000)
RATES = (0.0, 0.02, 0.05, 0.10, 0.15)
ACGT = list(b"ACGT")
# the batch at size of the GPU test: 150-base patterns in 400-base texts at 4 %, bound 12
BIG = dict(count=20_000, m=150, n=400, rate=0.04, bound=12, seed=99, sample=200)


def _rand(rng, n, alphabet=ACGT):
    return [alphabet[int(x)] for x in rng.integers(0, len(alphabet), n)]


def mutate(rng, seq, rate, alphabet=ACGT):
    """`seq` with round(rate * len) edits: substitutions, insertions and deletions in equal parts"""
    t = list(seq)
    for _ in range(int(round(rate * len(seq)))):
        kind = int(rng.integers(0, 3))
        if kind == 1 or not t:
            t.insert(int(rng.integers(0, len(t) + 1)), alphabet[int(rng.integers(0, len(alphabet)))])
            continue
        pos = int(rng.integers(0, len(t)))
        if kind == 0:
            t[pos] = alphabet[(alphabet.index(t[pos]) + 1 + int(rng.integers(0, len(alphabet) - 1))) % len(alphabet)]
        else:
            del t[pos]
    return t


def plant(rng, pattern, n, where, rate, alphabet=ACGT):
    """a text of exactly n symbols holding a mutated copy of the pattern: at the text's start (where 0), at its end (1), or
    across a column-64 boundary (2); a copy longer than the text is cut to n symbols from its start / end / middle"""
    occ = mutate(rng, pattern, rate, alphabet)
    if len(occ) >= n:
        off = 0 if where == 0 else (len(occ) - n if where == 1 else (len(occ) - n) // 2)
        return bytes(occ[off:off + n])
    flank = n - len(occ)
    if where == 0:
        at = 0
    elif where == 1:
        at = flank
    else:                                         # the copy's middle on the first column-64 boundary it can reach
        at = min(flank, max(0, 64 * max(1, (len(occ) // 2 + 63) // 64) - len(occ) // 2))
    left = _rand(rng, at, alphabet)
    if left and len(pattern) <= 2:                # a pattern this short has a match at the text's start too: d < m in PREFIX mode
        left[0] = pattern[0]
    return bytes(left + occ + _rand(rng, flank - at, alphabet))


def grid_cases():
    """[(pattern, text)]: every (m, n) of M_LENS x N_LENS with the match at the start, at the end and across a column-64
    boundary; the planted edit rate rotates through RATES"""
    rng = np.random.default_rng(SEED)
    out, v = [], 0
    for m in M_LENS:
        for n in N_LENS:
            for where in (0, 1, 2):
                pattern = bytes(_rand(rng, m))
                out.append((pattern, plant(rng, pattern, n, where, RATES[v % len(RATES)])))
                v += 1
    return out


def tie_cases():
    """two occurrences of equal cost (the smallest end); matches that may start with an insertion or a mismatch (the longest
    stretch)"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for m in (10, 64, 70, 130):
        p = bytes(_rand(rng, m))
        for gap in (0, 1, 30, 64, 100):
            f = [bytes(_rand(rng, k)) for k in (int(rng.integers(0, 70)), gap, int(rng.integers(0, 70)))]
            out.append((p, f[0] + p + f[1] + p + f[2]))
            q = bytearray(p)
            q[m // 2] = ACGT[(ACGT.index(q[m // 2]) + 1) % 4]
            out.append((p, f[0] + bytes(q) + f[1] + bytes(q) + f[2]))          # both with one mismatch
    out += [(b"CACGT", b"TTGACGT"), (b"CACGT", b"TTACGT"), (b"AACGT", b"GGAACGTAACGT"), (b"ACGTACGT", b"TTTCGTACGTTT"),
            (b"GATTACA", b"CCGTTACAGATACA"), (b"ACACACAC", b"TTACACACACACACTT"), (b"A" * 64 + b"C", b"G" + b"A" * 70 + b"C" + b"A" * 70),
            (b"TTTTT", b"TTTTTTTTTTTT"), (b"ACGT" * 20, b"ACGT" * 50)]
    return out


def no_similarity_cases():
    """the named cases without any similarity: d == m in both modes, edlib's end location -1"""
    return [(b"A", b"C"), (b"AC", b"GGGG"), (b"A" * 65, b"C" * 130)]


LIVE_SHAPES = ((1000, 3000), (3000, 8000))
LIVE_BOUNDS = (20, 100)


def live_cases():
    """long patterns for the live-block rule: [(pattern, text, bound, at)], one case per shape of LIVE_SHAPES x bound of
    LIVE_BOUNDS x decoy x indel.  The real occurrence starts at `at`, past the text's middle, and costs at most the bound:
    without indels bound / 2 substitutions; with indels no substitution but a deletion and, further on, an insertion of
    g = min(m / 20, bound / 2) bases each (at most 2 g <= bound edits; the live region has to grow and shrink).  The decoy is
    a copy of the pattern with bound + 6 substitutions ahead of the real occurrence -- just beyond the bound, so a sweep that
    is right passes it by and one that keeps too few blocks alive loses the real one behind it.  The tests assert on the
    brute force that the real occurrence is within the bound and that nothing before `at` is."""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for m, n in LIVE_SHAPES:
        for bound in LIVE_BOUNDS:
            for decoy in (0, 1):
                for indel in (0, 1):
                    p = _rand(rng, m)
                    occ = list(p)
                    if indel:
                        g = min(m // 20, bound // 2)
                        a, b = m // 3, 2 * m // 3
                        occ = occ[:a] + occ[a + g:b] + _rand(rng, g) + occ[b:]
                    else:
                        for pos in rng.choice(m, size=bound // 2, replace=False):
                            occ[pos] = ACGT[(ACGT.index(occ[pos]) + 1) % 4]
                    at = n // 2 + int(rng.integers(0, 64))
                    text = _rand(rng, n)
                    text[at:at + len(occ)] = occ
                    if decoy:
                        d = list(p)
                        for pos in rng.choice(m, size=bound + 6, replace=False):
                            d[pos] = ACGT[(ACGT.index(d[pos]) + 1) % 4]
                        lo = 10 + int(rng.integers(0, 64))
                        assert lo + m + bound < at
                        text[lo:lo + m] = d
                    assert len(text) == n
                    out.append((bytes(p), bytes(text), bound, at))
    return out


def random_cases(count=2000):
    """[(pattern, text, mode, bound)]: random shapes, planted rates and bounds"""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for i in range(count):
        m = int(rng.integers(1, 301)) if i % 4 else int(rng.integers(1, 70))
        n = int(rng.integers(1, 401))
        p = bytes(_rand(rng, m))
        t = plant(rng, p, n, int(rng.integers(0, 3)), float(rng.choice(RATES)) if i % 7 else 0.4)
        bound = int(rng.choice((0, 1, 2, 5, 12, 30, 63, 64, 65, 128, m, 2**31 - 1)))
        out.append((p, t, PREFIX if i % 2 else INFIX, bound))
    return out


def symbol_cases():
    """N, lower-case and IUPAC bytes (the brute force alone judges these)"""
    rng = np.random.default_rng(SEED + 4)
    out = []
    for i in range(48):
        alphabet = [list(b"ACGTN"), list(b"ACGTacgt"), list(b"ACGTRYKMN"), list(b"ACGTacgtNnRy")][i % 4]
        m = int(rng.integers(1, 200))
        p = bytes(_rand(rng, m, alphabet))
        out.append((p, plant(rng, p, int(rng.integers(m, m + 200)), i % 3, RATES[i % len(RATES)], alphabet)))
    return out


_big = []


def big_batch():
    """the batch at size as [(pattern, text)]: a mutated copy of every pattern at a random place of its text"""
    if not _big:
        rng = np.random.default_rng(BIG["seed"])
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        pats = lut[rng.integers(0, 4, (BIG["count"], BIG["m"]))]
        flanks = lut[rng.integers(0, 4, (BIG["count"], BIG["n"]))]
        for i in range(BIG["count"]):
            p = pats[i].tobytes()
            occ = bytes(mutate(rng, p, BIG["rate"]))
            at = int(rng.integers(0, BIG["n"] - len(occ) + 1))
            f = flanks[i].tobytes()
            _big.append((p, f[:at] + occ + f[at:BIG["n"] - len(occ)]))
    return _big


def big_sample_indices():
    return sorted(int(x) for x in np.random.default_rng(SEED + 5).choice(BIG["count"], size=BIG["sample"], replace=False))


SETS = {"grid": lambda: [(p, t) for p, t in grid_cases()], "ties": lambda: [(p, t) for p, t in tie_cases()], "no_similarity": no_similarity_cases,
        "live": lambda: [(c[0], c[1]) for c in live_cases()], "random": lambda: [(p, t) for p, t, _, _ in random_cases()],
        "big_sample": lambda: [big_batch()[i] for i in big_sample_indices()]}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def expected(name):
    """edlib's [[d, start, end] for SHW, [..] for HW] per case of a set: live where oracle/_ref is built (and then equal to
    the record), else the record"""
    import search_lib as S
    rec = load()[name]
    pairs = SETS[name]()
    assert len(rec) == len(pairs), f"{FIXTURE}[{name}] is stale: regenerate it"
    if not S.have_edlib():
        return rec
    live = [[S.edlib_locate(p, t, PREFIX), S.edlib_locate(p, t, INFIX)] for p, t in pairs]
    assert live == rec, f"{FIXTURE}[{name}] differs from the live oracle: regenerate it"
    return live


def main():
    import search_lib as S
    assert S.have_edlib(), "build oracle/_ref first (make -C oracle ref)"
    out = {"seed": SEED}
    for name, make in SETS.items():
        out[name] = [[S.edlib_locate(p, t, PREFIX), S.edlib_locate(p, t, INFIX)] for p, t in make()]
        print(name, len(out[name]), "cases")
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
