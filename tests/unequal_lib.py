"""Pairs of unequal lengths inside the reference's own domain: the grid, the parameter sets and the domain rule that
tests/test_oracle_vs_ref.py (oracle against the compiled reference), tests/test_gpu_unequal.py (every kernel form against
the oracle) and tests/test_narrow_cpu.py (the CPU model of the score-only walk) share.  Test infrastructure only.

The length difference is an input of the band geometry (bpm_banded.c:123-133: relative cutoff, prologue blocks, effective
bandwidth, the last block's position inside the band); datagen's pairs keep it at the few values that their errors give.

THE DOMAIN.  The compiled reference computes nothing outside it, so nothing here leaves it:
  * the text (the second sequence) is less than three times the pattern: beyond, the reference dies (SIGSEGV in BANDED,
    HIRSCHBERG and QUICKED).  The grid's ratios stop at 2;
  * score-only BANDED with the band below the true distance: the reference returns a negative number of no meaning, the
    oracle the -1 of DESIGN.md 5;
  * BANDED / HIRSCHBERG with a CIGAR and the band below the true distance: score and CIGAR differ."""
from quicked_amd import datagen

LENGTHS = (64, 65, 127, 128, 129, 200, 500, 1000, 2500)                                   # the pattern's length m
RATIOS = ((1, 2), (2, 3), (4, 5), (9, 10), (11, 10), (5, 4), (3, 2), (2, 1))                # text length / m
SHAPES = ("tail", "mid")
ERROR = 0.03
SEED = 7000

QUICKED, WINDOWED, BANDED, HIRSCHBERG = 0, 1, 2, 3

# name -> parameters (oracle_lib.oracle_align, oracle_lib.ref_expected and capi.make_params take the same keywords)
PARAM_SETS = {
    "banded_so_bw15": dict(algo=BANDED, only_score=True, bandwidth=15),
    "banded_so_bw40": dict(algo=BANDED, only_score=True, bandwidth=40),
    "banded_so_bw100": dict(algo=BANDED, only_score=True, bandwidth=100),
    "banded_so_bw15_scalar": dict(algo=BANDED, only_score=True, bandwidth=15, force_scalar=True),
    "banded_bw15": dict(algo=BANDED, bandwidth=15),
    "banded_bw40": dict(algo=BANDED, bandwidth=40),
    "banded_bw100": dict(algo=BANDED, bandwidth=100),
    "hirschberg_bw40": dict(algo=HIRSCHBERG, bandwidth=40),
    "hirschberg_bw100": dict(algo=HIRSCHBERG, bandwidth=100),
    "windowed_so": dict(algo=WINDOWED, only_score=True),
    "windowed": dict(algo=WINDOWED),
    "windowed_w2": dict(algo=WINDOWED, window_size=2),
    "windowed_w2_scalar": dict(algo=WINDOWED, window_size=2, force_scalar=True),
    "quicked": dict(algo=QUICKED),
    "quicked_scalar": dict(algo=QUICKED, force_scalar=True),
}
# The sets whose score is the exact distance on every pair inside the domain: QuickEd, BandEd and Hirschberg with a CIGAR
# (the domain rule is "the band holds the distance") and score-only BandEd at bandwidth 100 (the cutoff is the longer
# sequence: no distance is above it).  The others are heuristics in the reference itself and overshoot on this grid, the
# oracle with them, score for score: score-only BandEd cuts its band's edges by scores that a length difference inflates
# (500 x 550 at bandwidth 15: 78 from both, the distance is 64, the cutoff 82), WindowEd follows one window's traceback
# (500 x 750 at the default window: 301 against 267; 71 of 144 pairs at window_size = 2).  For them oracle == reference
# is the check, and score >= distance.
EXACT_SETS = ("banded_so_bw100", "banded_bw15", "banded_bw40", "banded_bw100", "hirschberg_bw40", "hirschberg_bw100",
              "quicked", "quicked_scalar")

# pairs of the 144 that the domain rule leaves per set.  Score-only BandEd: a negative score needs a pattern longer than
# its text (9 pairs at bandwidth 15, 7 at 40); with a CIGAR the rule is distance <= cutoff, and on this grid the length
# difference alone is above 15 % of the longer sequence for every ratio but 9/10 and 11/10 (2 x 2 x 9 = 36 pairs at the
# most), above 40 % for the ratios 1/2 and 2 (36 pairs out at the least).  The figures are the grid's own, pinned so that
# neither the grid nor the rule can shrink unseen.
MIN_INSIDE = dict({k: 144 for k in PARAM_SETS}, banded_so_bw15=135, banded_so_bw15_scalar=135, banded_so_bw40=137,
                  banded_bw15=35, banded_bw40=108, hirschberg_bw40=108)

_grid = None


def _cut(seq, keep, shape):
    """`seq` shortened to `keep` bases: tail keeps the prefix, mid takes the surplus out of the middle (one large indel)"""
    if shape == "tail":
        return seq[:keep]
    head = keep // 2
    return seq[:head] + seq[len(seq) - (keep - head):]


def grid():
    """-> [(pattern, text, shape)]: 9 pattern lengths x 8 ratios x 2 shapes = 144 pairs, case k = 1 .. 144 in that nesting
    order from datagen.generate(1, max(m, n), 0.03, seed=7000 + k); the sequence that has to be the shorter one is cut to
    its length, the other stays as generated (a generated pattern is its text's length give or take its indel errors)"""
    global _grid
    if _grid is None:
        out, k = [], 0
        for m in LENGTHS:
            for num, den in RATIOS:
                n = m * num // den
                for shape in SHAPES:
                    k += 1
                    p, t = next(datagen.generate(1, max(m, n), ERROR, seed=SEED + k).pairs())
                    if n < m:
                        t = _cut(t, n, shape)
                    else:
                        p = _cut(p, m, shape)
                    out.append((p, t, shape))
        _grid = out
    return list(_grid)


def pairs():
    return [(p, t) for p, t, _ in grid()]


def makes_cigar(kw):
    return not kw.get("only_score", False)


def band_holds(kw, m, n, exact):
    """the band of BANDED / HIRSCHBERG at this bandwidth holds an optimal path (quicked.c:64: the cutoff); true for the
    algorithms that choose their own band"""
    return kw["algo"] not in (BANDED, HIRSCHBERG) or exact <= max(m, n) * kw["bandwidth"] // 100


def in_domain(kw, m, n, exact, oracle_score):
    """one rule for the CPU and the GPU half.  kw: the parameter set; m, n: the lengths; exact: the full-height distance
    (qo_exact_distance); oracle_score: the oracle's score under kw"""
    if kw["algo"] in (BANDED, HIRSCHBERG):
        if makes_cigar(kw):
            return band_holds(kw, m, n, exact)                            # the rule of tests/test_gpu_parity.py
        if kw["algo"] == BANDED:
            return oracle_score >= 0                                      # below the distance: -1 here, garbage there
    return True
