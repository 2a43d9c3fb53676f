"""BandEd score-only in two passes, modelled with the oracle: what the CPU property test and the GPU
tests of QE_SCORE_NARROW compare with.  Test infrastructure only."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O
from native_build import host_lib
from quicked_amd import datagen


def max_cutoff(m, n, bandwidth):
    return (max(m, n) * bandwidth) // 100                  # quicked.c:64


def effective(m, n, cutoff):
    return max(abs(n - m) + 1, cutoff, 65)                 # banded_matrix_allocate's clamps


def slots(m, n, cutoff):
    """slots of the score-only band (bpm_banded.c:801-803)"""
    return ((effective(m, n, cutoff) + 63) >> 6) + 1


def cover(m, n, cutoff):
    """diagonals below the main one that the score-only band at this cutoff holds in every column (qe_types.h: narrow_cover)"""
    ce, diff = effective(m, n, cutoff), m - n
    rel = (ce - abs(diff) + 1) // 2
    prolog = (rel + max(0, -diff) + 63) // 64
    return 64 * (((ce + 63) >> 6) - prolog)


def accepts(m, n, c1, cutoff, r):
    """the first pass's result stands for the pass at `cutoff`: the cost of a path within c1, and both bands hold every
    diagonal a path of that cost can touch (qe_types.h: narrow_accepts)"""
    diff = m - n
    if r < abs(diff) or r > c1:
        return False
    return max(0, diff) + (r - abs(diff)) // 2 <= min(cover(m, n, c1), cover(m, n, cutoff))


def narrow_cutoff(m, n, cutoff):
    """the cutoff of a task's first pass: half, where that band has fewer slots; else the task has one pass only"""
    half = cutoff // 2
    return half if slots(m, n, half) < slots(m, n, cutoff) else cutoff


def banded_score(p, t, cutoff):
    adv = C.c_int64(0)
    sc = O.oracle().qo_banded_score(p, len(p), t, len(t), cutoff, len(t), None, None, C.byref(adv))
    return int(sc), int(adv.value)


def two_pass(p, t, cutoff):
    """-> dict: the single pass at `cutoff` (score, adv), the first pass at the halved cutoff (score1, adv1, cut1),
    whether it was accepted, whether the task has a second pass (miss), the block-columns both passes advance (adv2p)"""
    m, n = len(p), len(t)
    sc, adv = banded_score(p, t, cutoff)
    c1 = narrow_cutoff(m, n, cutoff)
    if c1 == cutoff:
        return dict(score=sc, adv=adv, cut1=c1, score1=sc, adv1=adv, narrower=False, accepted=True, miss=False, adv2p=adv)
    s1, a1 = banded_score(p, t, c1)
    ok = accepts(m, n, c1, cutoff, s1)
    return dict(score=sc, adv=adv, cut1=c1, score1=s1, adv1=a1, narrower=True, accepted=ok, miss=not ok,
                adv2p=a1 + (0 if ok else adv))


def two_pass_many(pairs, bandwidth=15, cutoffs=None):
    threads = max(1, min(32, len(os.sched_getaffinity(0))))
    O.oracle()
    if cutoffs is None:
        cutoffs = [max_cutoff(len(p), len(t), bandwidth) for p, t in pairs]
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda a: two_pass(a[0][0], a[0][1], a[1]), zip(pairs, cutoffs)))


PROBE = 16          # qe_stages.hip: QE_NARROW_PROBE -- every 16th eligible run probes, on every 16th group of 64 tasks


def library_order(pairs):
    """the order the library's task list holds the pairs in (batch_load: a stable sort by max(m, n), longest first)"""
    return sorted(range(len(pairs)), key=lambda i: -max(len(pairs[i][0]), len(pairs[i][1])))


def probe_expectation(pairs, res):
    """block-columns of a probe run: the single pass for every task, and beside it the pass at the halved cutoff for the
    tasks of every PROBE-th group whose band is narrower there (no second-pass task: no result depends on a probe)"""
    adv = 0
    for t, i in enumerate(library_order(pairs)):
        r = res[i]
        adv += r["adv"]
        if (t >> 6) % PROBE == 0 and r["narrower"]:
            adv += r["adv1"]
    return adv


def native_rule(tmp_dir):
    """qe_types.h's narrow_cutoff / narrow_cover / narrow_accepts compiled for the host (the header is plain C++ there)"""
    return host_lib(tmp_dir, "narrow_rule",
                    'extern "C" int nr_cutoff(int m, int n, int c) { return qe::narrow_cutoff(m, n, c); }\n'
                    'extern "C" int nr_cover(int m, int n, int c) { return qe::narrow_cover(m, n, c); }\n'
                    'extern "C" int nr_slots(int m, int n, int c) { return qe::narrow_slots(m, n, c); }\n'
                    'extern "C" int nr_accepts(int m, int n, int c1, int c, int r) { return qe::narrow_accepts(m, n, c1, c, r) ? 1 : 0; }\n')


# The grid of shapes the property is checked on (committed: the lists below ARE the cases).
LENGTHS = (200, 1000, 3000, 10000)
ERRORS = (0.01, 0.03, 0.05, 0.07, 0.074, 0.076, 0.08, 0.10, 0.14)
PER_CELL = 46                                              # 4 x 9 x 2 x 46 = 3 312 pairs


def grid_pairs():
    """(label, pattern, text) over lengths x error rates, without and with two indels of length / 20"""
    for li, length in enumerate(LENGTHS):
        for ei, err in enumerate(ERRORS):
            for indel in (0, 1):
                b = datagen.generate(count=PER_CELL, length=length, error=err, seed=9000 + 100 * li + 2 * ei + indel,
                                     indels_num=2 * indel, indels_len=(length // 20) * indel)
                for i, (p, t) in enumerate(b.pairs()):
                    yield (length, err, indel, i), p, t


def ragged_pairs(bandwidth=15):
    """||m| - |n|| at and around C' = C / 2 (the corridor eats the whole first band) for texts of 1 000 and 3 000"""
    rng = np.random.default_rng(77)
    for length in (1000, 3000):
        base = datagen.generate(count=24, length=length, error=0.03, seed=9500 + length)
        for i, (p, t) in enumerate(base.pairs()):
            half = max_cutoff(len(p), len(t), bandwidth) // 2
            for k, delta in enumerate((half - 66, half - 2, half - 1, half, half + 1, half + 2, half + 66)):
                cut = min(max(delta, 0), len(p) - 1)
                if (i + k) % 2:
                    yield (length, "short-p", delta, i), p[cut:], t        # pattern shorter by ~delta
                else:
                    ins = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), cut))
                    yield (length, "long-p", delta, i), p[: len(p) // 2] + ins + p[len(p) // 2:], t


def symbol_pairs():
    """N, lower-case and IUPAC symbols in reads of 1 000 and 3 000 at error rates either side of the halved cutoff"""
    rng = np.random.default_rng(78)
    for length in (1000, 3000):
        for err in (0.03, 0.07, 0.09):
            b = datagen.generate(count=12, length=length, error=err, seed=9600 + length + int(err * 1000))
            for i, (p, t) in enumerate(b.pairs()):
                p, t = bytearray(p), bytearray(t)
                if i % 3 == 0:
                    for k in rng.integers(0, len(p), 4): p[k] = ord("N")
                    for k in rng.integers(0, len(t), 4): t[k] = ord("N")
                elif i % 3 == 1:
                    p = bytearray(bytes(p).lower())
                else:
                    for k in rng.integers(0, len(t), 3): t[k] = ord("R")
                    for k in rng.integers(0, len(p), 3): p[k] = ord("n")
                yield (length, err, "sym", i), bytes(p), bytes(t)


def floor_cutoffs():
    """explicit cutoffs whose halves lie at and around the floor of 65 and around multiples of 64, on reads of 1 500 at 2 %"""
    b = datagen.generate(count=8, length=1500, error=0.02, seed=9700)
    prs = list(b.pairs())
    for c in (126, 128, 129, 130, 131, 132, 134, 190, 192, 194, 254, 256, 257, 258, 260, 382, 384, 386, 510, 512, 514):
        for i, (p, t) in enumerate(prs):
            yield (c, i), p, t, c


def random_shapes(seed=1, rounds=200):
    """(pattern, text, cutoff): random lengths 100 .. 3 000, error rates, indels, clipped ends (ragged pairs either way
    round) and three random cutoffs 66 .. 1 200 per pair -- where "0 <= r' <= C'" alone fails on ~0.3 % of the cases"""
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        length = int(rng.integers(100, 3000))
        err = float(rng.choice([0.005, 0.01, 0.02, 0.04, 0.06, 0.08, 0.12]))
        ind = int(rng.integers(0, 3))
        il = int(rng.integers(1, max(2, length // 10)))
        b = datagen.generate(count=6, length=length, error=err, seed=int(rng.integers(1, 1 << 30)), indels_num=ind,
                             indels_len=il if ind else 0)
        for p, t in b.pairs():
            if rng.integers(0, 2):
                p, t = t, p
            k = int(rng.integers(0, 4))
            if k == 1:
                p = p[int(rng.integers(0, min(len(p) - 1, 200))):]
            if k == 2:
                t = t[: len(t) - int(rng.integers(0, min(len(t) - 1, 200)))]
            if len(p) == 0 or len(t) == 0:
                continue
            for c in rng.integers(66, min(1200, 2 * max(len(p), len(t))), 3):
                yield p, t, int(c)
