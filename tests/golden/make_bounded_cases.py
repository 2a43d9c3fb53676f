"""The fixed cases of the bounded-distance tests (tests/test_bounded_cpu.py, tests/test_gpu_bounded.py) and the recorder of
their expected distances.

The sequences are regenerated from seeds by the functions below, which the tests import; only the DISTANCES are recorded,
in tests/golden/bounded_cases.json: upper-case ACGT / ACGTN cases from edlib (global distance; N is a symbol like any
other there, which is the library's rule for upper-case ACGTN), cases with lower-case / IUPAC bytes from the compiled
reference's algo = QUICKED score.  Neither comes from the library under test.  Where oracle/_ref is built the tests use
the live values and require them to equal this record; where it is not, the record alone.

    python tests/golden/make_bounded_cases.py        # needs oracle/_ref (make -C oracle ref)
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

FIXTURE = os.path.join(HERE, "bounded_cases.json")
SEED = 20261016
LENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
MAX_DIAG = 63                                   # the largest bound the diagonal-word kernel takes
SUBS = (0, 1, 2, 4, 7, 12, 20, 33, 50, 70, 100, 126)     # planted substitutions: 0 .. 2 k for k = 63
# the bounds of the second GPU batch: 0, small, around the kernel's limit, large, and "above max(m, n)" (-1 here)
MIXED_BOUNDS = (0, 3, 9, 24, 63, 64, 65, 100, 1000, -1)
# the batch at size: 100 000 pairs of 10 kb in seven equal segments with 12 .. 48 planted edits each (0.3 % on average), so
# that a bound at the median distance has pairs on both sides
BIG = dict(count=100_000, length=10_000, edits=(12, 20, 26, 30, 34, 40, 48), seed=77, sample=200)


def big_segments():
    """[(first pair, pairs, planted edits)]"""
    k = len(BIG["edits"])
    per = BIG["count"] // k
    return [(s * per, per if s < k - 1 else BIG["count"] - s * per, e) for s, e in enumerate(BIG["edits"])]


def big_batch():
    from quicked_amd import datagen
    out = None
    for s, (first, count, edits) in enumerate(big_segments()):
        b = datagen.generate(count, BIG["length"], float(edits), seed=BIG["seed"] + s)
        out = b if out is None else out.concat(b)
    return out


def _mutate(rng, pattern, n, where, subs, alphabet):
    """text of exactly n symbols from `pattern`: one run of |m - n| deletions / insertions at the start (where 0), at the
    end (1) or at a random place (2), then `subs` substitutions at distinct places"""
    m = len(pattern)
    t = list(pattern)
    gap = abs(m - n)
    if n < m:
        at = 0 if where == 0 else (m - gap if where == 1 else int(rng.integers(0, m - gap + 1)))
        del t[at:at + gap]
    elif n > m:
        at = 0 if where == 0 else (m if where == 1 else int(rng.integers(0, m + 1)))
        t[at:at] = [alphabet[int(x)] for x in rng.integers(0, len(alphabet), gap)]
    for pos in rng.choice(n, size=min(subs, n), replace=False):
        t[pos] = alphabet[(alphabet.index(t[pos]) + 1 + int(rng.integers(0, len(alphabet) - 1))) % len(alphabet)]
    return bytes(t)


def grid_pairs():
    """[(pattern, text)]: every (m, n) of LENS x LENS in six variants -- the place of the insertion / deletion run x two
    substitution counts that rotate through SUBS, alternating ACGT and ACGTN -- then the special pairs"""
    rng = np.random.default_rng(SEED)
    out = []
    v = 0
    for m in LENS:
        for n in LENS:
            for where in (0, 1, 2):
                for _ in range(2):
                    alphabet = list(b"ACGT") if v % 2 == 0 else list(b"ACGTN")
                    pattern = bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), m))
                    out.append((pattern, _mutate(rng, pattern, n, where, SUBS[v % len(SUBS)], alphabet)))
                    v += 1
    for k in (1, 40, 64, 200):                   # identical pairs; pairs without a common base
        s = bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        out.append((s, s))
        out.append((b"A" * k, b"C" * k))
    out.append((b"ACGT" * 16, b"ACGT" * 16 + b"T" * 63))      # pure insertion run of the largest bound, at the end
    out.append((b"G" * 63 + b"ACGT" * 16, b"ACGT" * 16))      # pure deletion run, at the start
    return out


def long_pairs():
    """10 kb pairs with 0, 1, ~40, ~60 and ~90 planted edits (substitutions, insertions and deletions)"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for edits in (0, 1, 40, 60, 90):
        p = list(rng.choice(list(b"ACGT"), 10_000).astype(np.uint8))
        t = list(p)
        for _ in range(edits):
            kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(t)))
            if kind == 0:
                t[pos] = b"ACGT"[(b"ACGT".index(t[pos]) + 1 + int(rng.integers(0, 3))) % 4]
            elif kind == 1:
                t.insert(pos, int(rng.choice(list(b"ACGT"))))
            else:
                del t[pos]
        out.append((bytes(p), bytes(t)))
    return out


def noncanon_pairs():
    """pairs with N, lower-case and IUPAC bytes (expected: the reference's QUICKED score)"""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for i in range(48):
        m = int(rng.integers(40, 400))
        alphabet = [list(b"ACGTN"), list(b"ACGTacgt"), list(b"ACGTRYKMN"), list(b"ACGTacgtNnRy")][i % 4]
        p = bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), m))
        n = max(1, m + int(rng.integers(-6, 7)))
        out.append((p, _mutate(rng, p, n, i % 3, int(rng.integers(0, 30)), alphabet)))
    return out


def mixed_bounds(pairs):
    """per-pair bounds of the second GPU batch"""
    return [max(len(p), len(t)) + 7 if MIXED_BOUNDS[i % len(MIXED_BOUNDS)] < 0 else MIXED_BOUNDS[i % len(MIXED_BOUNDS)]
            for i, (p, t) in enumerate(pairs)]


def big_sample_indices():
    return sorted(int(x) for x in np.random.default_rng(SEED + 3).choice(BIG["count"], size=BIG["sample"], replace=False))


def big_sample_pairs():
    """the sampled pairs of the batch at size, generated one by one (pair i depends on (seed, i) only)"""
    from quicked_amd import datagen
    out = []
    segs = big_segments()
    for i in big_sample_indices():
        s = max(q for q, (first, _, _) in enumerate(segs) if first <= i)
        b = datagen.generate(1, BIG["length"], float(segs[s][2]), seed=BIG["seed"] + s, first=i - segs[s][0])
        out.append((b.pattern(0), b.text(0)))
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def expected(name, pairs, noncanon=False):
    """the distances of a case set: live where oracle/_ref is built (and then equal to the record), else the record"""
    import oracle_lib as O
    rec = load()[name]
    assert len(rec) == len(pairs), f"{FIXTURE}[{name}] is stale: regenerate it"
    have = O.have_ref() if noncanon else O.have_edlib()
    if not have:
        return list(rec)
    live = [O.ref_align(p, t)[1] for p, t in pairs] if noncanon else [O.edlib_distance(p, t) for p, t in pairs]
    assert live == list(rec), f"{FIXTURE}[{name}] differs from the live oracle: regenerate it"
    return live


def threshold(d, bound):
    return d if d <= bound else -1


def _balance(name, exp):
    n, within = len(exp), sum(1 for e in exp if e >= 0)
    print(f"{name}: {n} entries, {within / n:.1%} within, {(n - within) / n:.1%} beyond")
    assert within * 4 >= n and (n - within) * 4 >= n, name


def main():
    import oracle_lib as O
    assert O.have_edlib() and O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    out = {"seed": SEED}
    g = grid_pairs()
    out["grid"] = [O.edlib_distance(p, t) for p, t in g]
    out["long"] = [O.edlib_distance(p, t) for p, t in long_pairs()]
    out["noncanon"] = [O.ref_align(p, t)[1] for p, t in noncanon_pairs()]
    out["big_sample"] = [O.edlib_distance(p, t) for p, t in big_sample_pairs()]
    # the conditions the GPU batches assert, checked here on the oracle's distances alone
    _balance("grid x bounds 0..63", [threshold(d, k) for d in out["grid"] for k in range(MAX_DIAG + 1)])
    _balance("grid, mixed bounds", [threshold(d, k) for d, k in zip(out["grid"], mixed_bounds(g))])
    nc = noncanon_pairs()
    _balance("noncanon", [threshold(d, k) for d, k in zip(out["noncanon"], noncanon_bounds(out["noncanon"]))])
    med = int(np.median(out["big_sample"]))
    _balance("big sample at its median", [threshold(d, med) for d in out["big_sample"]])
    del nc
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


def noncanon_bounds(dist):
    """bounds of the non-canonical batch: alternately just below and at / above each pair's recorded distance"""
    return [max(0, d - 1 - i % 3) if i % 2 else d + i % 4 for i, d in enumerate(dist)]


if __name__ == "__main__":
    main()
