"""The fixed cases of the all-occurrences tests (tests/test_search_hits_cpu.py, tests/test_gpu_search_hits.py) and the
recorder of the answers to them.

The sequences are regenerated from seeds: the grid, tie and random cases of make_search_cases.py, and below the shapes at which
the all-occurrences scan can go wrong.  Recorded in tests/golden/search_hits_cases.json, per case and mode (PREFIX, INFIX):
the brute force's occurrences without a bound ([[text_start, text_end, score]]; the occurrences at a bound k are those of
score <= k: the definition's other two conditions do not know k) and, for upper-case ACGT cases with d != m, edlib's view of
the occurrences of the best score ([d, [[start, end]]], search_hits_lib.edlib_best_occurrences; else null).  The tests compute
the brute force live and require the record to equal it; edlib is asked live where oracle/_ref is built, and then has to
equal the record too.

    python tests/golden/make_search_hits_cases.py        # needs oracle/_ref (make -C oracle ref)
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


def _base():
    spec = importlib.util.spec_from_file_location("make_search_cases", os.path.join(HERE, "make_search_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _base()
FIXTURE = os.path.join(HERE, "search_hits_cases.json")
SEED = 20261019
PREFIX, INFIX = 1, 2
ACGT = M.ACGT
DEAD_BOUND = 20
RANDOM_COUNT = 400


def _other(c):
    return ACGT[(ACGT.index(c) + 1) % 4]


def plateau_text(rng, q, first_end, n):
    """a text of n bases in which q ends at column first_end (1-based) and is followed by the two bases {x, a} with a != x:
    for the pattern q + a row m reads the same value after q (a deleted), after q x (a against x) and after q x a (x
    inserted) -- a plateau of three columns whose first one is first_end"""
    a = ACGT[int(rng.integers(0, 4))]
    x = _other(a)
    lead = first_end - len(q)
    assert lead >= 0 and first_end + 2 <= n
    return bytes(q + [a]), bytes(M._rand(rng, lead) + q + [x, a] + M._rand(rng, n - first_end - 2))


def border_cases():
    """plateaus that straddle columns 64 / 65 and 128 / 129 (and their neighbours)"""
    rng = np.random.default_rng(SEED)
    out = []
    for border in (64, 128):
        for first_end in (border - 1, border):
            for m in (20, 50, 61):
                out.append(plateau_text(rng, M._rand(rng, m - 1), first_end, 200))
    return out


def edge_cases():
    """a valley still pending at the text's last column (a plateau, and a descent in the very last column), and one at e = 1"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for m, n in ((20, 64), (20, 65), (70, 128), (70, 200), (130, 256)):
        q = M._rand(rng, m - 1)
        a = ACGT[int(rng.integers(0, 4))]
        out.append((bytes(q + [a]), bytes(M._rand(rng, n - m) + q + [_other(a)])))          # the plateau reaches the end
        p = M._rand(rng, m)
        out.append((bytes(p), bytes(M._rand(rng, n - m) + p)))                             # the descent to 0 in the last column
        out.append((bytes(p), bytes(p[-1:] + [_other(p[-1])] * 3 + M._rand(rng, n - 4))))  # the pattern's last base in column 1
    out += [(b"A", b"ACCC"), (b"A", b"A"), (b"AC", b"ATTT"), (b"AC", b"A"), (b"ACG", b"GTTTTTTG"), (b"T", b"TTTT"), (b"TG", b"TGTGTGTG")]
    return out


def short_text_cases():
    """texts shorter than the pattern"""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for m in (5, 64, 65, 130, 300):
        p = M._rand(rng, m)
        for n in (1, 2, m // 2, m - 1):
            at = int(rng.integers(0, m - n + 1))
            out.append((bytes(p), bytes(M.mutate(rng, p[at:at + n], 0.03)[:n] or p[:1])))
    return out


def tandem_cases():
    """a 16-base pattern in a 1 000-base text of its own repeat with 3 % errors: dozens of occurrences"""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for _ in range(3):
        p = M._rand(rng, 16)
        t = M.mutate(rng, p * 63, 0.03)
        out.append((bytes(p), bytes((t + p * 2)[:1000])))
    return out


def adjacent_cases():
    """two and three planted occurrences with fewer than m columns between them"""
    rng = np.random.default_rng(SEED + 4)
    out = []
    for m in (20, 64, 100, 150):
        p = M._rand(rng, m)
        for copies in (2, 3):
            for rate in (0.0, 0.04):
                t = M._rand(rng, int(rng.integers(0, 70)))
                for c in range(copies):
                    if c:
                        t += M._rand(rng, int(rng.integers(0, m)))
                    t += M.mutate(rng, p, rate)
                out.append((bytes(p), bytes(t + M._rand(rng, int(rng.integers(0, 70))))))
    return out


def length_cases():
    """the register form's limits: patterns of 1, 63, 64, 65, 256, 257 and 300 bases, two planted occurrences each"""
    rng = np.random.default_rng(SEED + 5)
    out = []
    for m in (1, 63, 64, 65, 256, 257, 300):
        for rate in (0.0, 0.05):
            p = M._rand(rng, m)
            t = M._rand(rng, 30) + M.mutate(rng, p, rate) + M._rand(rng, 90) + M.mutate(rng, p, rate) + M._rand(rng, 40)
            if m == 1:                            # a match at the text's start too: d < m in PREFIX mode, which edlib can judge
                t[0] = p[0]
            out.append((bytes(p), bytes(t)))
    return out


def dead_cases():
    """1 000-base patterns, two planted occurrences at 2 % error separated by 600 random columns, and a copy with
    DEAD_BOUND + 6 substitutions -- a decoy just beyond the bound -- ahead of, between or behind them: at bound DEAD_BOUND the
    lower blocks die between the occurrences and have to enter again"""
    rng = np.random.default_rng(SEED + 6)
    out = []
    for where in (0, 1, 2, 1):
        p = M._rand(rng, 1000)
        decoy = list(p)
        for pos in rng.choice(1000, size=DEAD_BOUND + 6, replace=False):
            decoy[pos] = _other(decoy[pos])
        parts = [M._rand(rng, 70), M.mutate(rng, p, 0.02), M._rand(rng, 600), M.mutate(rng, p, 0.02), M._rand(rng, 90)]
        parts.insert((0, 2, 4)[where] + 1, decoy + M._rand(rng, 300))
        out.append((bytes(p), bytes(sum(parts, []))))
    return out


def symbol_cases():
    """N, lower-case and IUPAC bytes, two planted occurrences each"""
    rng = np.random.default_rng(SEED + 7)
    out = []
    for i in range(16):
        alphabet = [list(b"ACGTN"), list(b"ACGTacgt"), list(b"ACGTRYKMN"), list(b"ACGTacgtNnRy")][i % 4]
        m = int(rng.integers(4, 150))
        p = M._rand(rng, m, alphabet)
        t = M._rand(rng, 20, alphabet) + M.mutate(rng, p, 0.04, alphabet) + M._rand(rng, 50, alphabet) + M.mutate(rng, p, 0.04, alphabet)
        out.append((bytes(p), bytes(t)))
    return out


SETS = {"grid": lambda: [(p, t) for p, t in M.grid_cases()], "ties": lambda: [(p, t) for p, t in M.tie_cases()],
        "random": lambda: [(p, t) for p, t, _, _ in M.random_cases(RANDOM_COUNT)],
        "borders": border_cases, "edges": edge_cases, "short": short_text_cases, "tandem": tandem_cases, "adjacent": adjacent_cases,
        "lengths": length_cases, "dead": dead_cases, "symbols": symbol_cases}
ACGT_ONLY = [name for name in SETS if name != "symbols"]


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def record_of(p, t, edlib):
    import search_hits_lib as H
    rec = []
    for mode in (PREFIX, INFIX):
        rec.append([list(o) for o in H.occurrences(p, t, mode, len(p))])
    for mode in (PREFIX, INFIX):
        e = H.edlib_best_occurrences(p, t, mode) if edlib else None
        rec.append(None if e is None else [e[0], e[1]])
    return rec


def main():
    import search_lib as S
    assert S.have_edlib(), "build oracle/_ref first (make -C oracle ref)"
    out = {"seed": SEED}
    for name, make in SETS.items():
        out[name] = [record_of(p, t, name in ACGT_ONLY) for p, t in make()]
        print(name, len(out[name]), "cases,", sum(len(r[1]) > 1 for r in out[name]), "with more than one INFIX occurrence")
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
