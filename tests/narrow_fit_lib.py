"""The fitted first pass of BandEd score-only in two passes (QE_NARROW_FIT), modelled with the oracle:
qe_types.h's narrow_fit_* restated in Python, the brute force they are checked against, and the model of a run -- groups of
64 tasks in library order, one slot count per group, the oracle's pass at every task's fitted cutoff, the rule, the pass at
C.  What the CPU tests and the GPU tests of the fit compare with.  Test infrastructure only."""
import os
from concurrent.futures import ThreadPoolExecutor

import narrow_lib as NL
import oracle_lib as O
from native_build import host_lib


def rhat(q, cutoff):
    """the result a fit at the ratio q (1/1024ths of the cutoff) is made for"""
    return (q * cutoff + 1023) >> 10


def room(m, n, c1, cutoff):
    """the largest result accepts(m, n, c1, cutoff, .) takes, -1 if none"""
    diff = m - n
    k = min(NL.cover(m, n, c1), NL.cover(m, n, cutoff)) - max(0, diff)
    if k < 0 or c1 < abs(diff):
        return -1
    return min(abs(diff) + 2 * k + 1, c1)


def floor_cutoff(m, n):
    return NL.effective(m, n, 0)


def fit_slots(m, n, cutoff, r_hat):
    diff = m - n
    if r_hat < abs(diff) or max(0, diff) + (r_hat - abs(diff)) // 2 > NL.cover(m, n, cutoff):
        return 0
    full = NL.slots(m, n, cutoff)
    for c in range(max(r_hat, floor_cutoff(m, n)), cutoff):
        s = ((c + 63) >> 6) + 1
        if s >= full:
            return 0
        if NL.accepts(m, n, c, cutoff, r_hat):
            return s
    return 0


def fit_cutoff(m, n, cutoff, s):
    if s >= NL.slots(m, n, cutoff):
        return 0
    best, best_room = 0, -2
    for c in range(max(64 * (s - 2) + 1, floor_cutoff(m, n)), min(64 * (s - 1), cutoff - 1) + 1):
        r = room(m, n, c, cutoff)
        if r > best_room:
            best, best_room = c, r
    return best


def fit_lane(m, n, cutoff, q, s_g):
    half = NL.narrow_cutoff(m, n, cutoff)
    if s_g <= 0 or s_g >= NL.slots(m, n, half):
        return half
    c = fit_cutoff(m, n, cutoff, s_g)
    return c if c > 0 and NL.accepts(m, n, c, cutoff, rhat(q, cutoff)) else half


def ratio(m, n, cutoff, r):
    """what a run reports of a lowered task's final score: ceil(1024 r / C) where the pass at C / 2 would have accepted it"""
    if not NL.accepts(m, n, NL.narrow_cutoff(m, n, cutoff), cutoff, r):
        return -1
    return (1024 * r + cutoff - 1) // cutoff


def brute_force(m, n, cutoff):
    """every cutoff below C, no shortcut: -> ([(cutoff, slots)] of the cutoffs whose band has fewer slots than C's; {slot count:
    the most any cutoff of that count accepts}; {slot count: the smallest cutoff at or above the floor that accepts that
    much})"""
    full, fl = NL.slots(m, n, cutoff), floor_cutoff(m, n)
    rows, most, where = [], {}, {}
    for c in range(1, cutoff):
        s = NL.slots(m, n, c)
        if s >= full:
            continue
        rows.append((c, s))
        top = -1
        for r in range(c, -1, -1):                            # the largest accepted result, by trying them all
            if NL.accepts(m, n, c, cutoff, r):
                top = r
                break
        if top > most.get(s, -2):
            most[s] = top
            where.pop(s, None)
        if c >= fl and top == most[s] and s not in where:
            where[s] = c
    return rows, most, where


def brute_least_slots(m, n, cutoff, rows, r_hat):
    """the least slot count among brute_force's cutoffs >= r_hat that accept r_hat, or 0"""
    return min([s for c, s in rows if c >= r_hat and NL.accepts(m, n, c, cutoff, r_hat)] + [1 << 30]) % (1 << 30)


def group_cutoffs(shapes, q):
    """shapes = [(m, n, cutoff)] in the order of the task list -> every task's first-pass cutoff: per group of 64 the largest
    fit_slots of its tasks that have one, then fit_lane (q = 0: C / 2 wherever that band is narrower)"""
    out = []
    for g in range(0, len(shapes), 64):
        grp = shapes[g:g + 64]
        s_g = max((fit_slots(m, n, c, rhat(q, c)) for m, n, c in grp), default=0) if q > 0 else 0
        out += [fit_lane(m, n, c, q, s_g) for m, n, c in grp]
    return out


def fit_model(pairs, q, bandwidth=15, cutoffs=None, memo=None):
    """a two-pass run whose first pass is fitted to q, pairs in the caller's order (grouped as the library orders them) ->
    per pair: the single pass (score, adv), the first pass (cut1, score1, adv1), lowered, miss, fit_miss (a miss the pass
    at C / 2 would not have had), adv2p (block-columns of both passes), ratio (what the run reports of it, -1: nothing).
    memo: a dict that keeps the oracle's passes between calls on the SAME list of pairs"""
    memo = {} if memo is None else memo

    def banded(i, c):
        if (i, c) not in memo:
            memo[(i, c)] = NL.banded_score(pairs[i][0], pairs[i][1], c)
        return memo[(i, c)]

    if cutoffs is None:
        cutoffs = [NL.max_cutoff(len(p), len(t), bandwidth) for p, t in pairs]
    order = NL.library_order(pairs)
    cut1 = [0] * len(pairs)
    for i, c1 in zip(order, group_cutoffs([(len(pairs[i][0]), len(pairs[i][1]), cutoffs[i]) for i in order], q)):
        cut1[i] = c1

    def one(i):
        p, t = pairs[i]
        m, n, c, c1 = len(p), len(t), cutoffs[i], cut1[i]
        sc, adv = banded(i, c)
        if c1 == c:
            return dict(score=sc, adv=adv, cut1=c1, score1=sc, adv1=adv, lowered=False, miss=False, fit_miss=False, adv2p=adv, ratio=-1)
        s1, a1 = banded(i, c1)
        ok = NL.accepts(m, n, c1, c, s1)
        rt = ratio(m, n, c, s1 if ok else sc)
        return dict(score=sc, adv=adv, cut1=c1, score1=s1, adv1=a1, lowered=True, miss=not ok, fit_miss=(not ok) and rt >= 0,
                    adv2p=a1 + (0 if ok else adv), ratio=rt)

    O.oracle()
    with ThreadPoolExecutor(max(1, min(32, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(one, range(len(pairs))))


def learned_q(res):
    """NarrowArgs::stat[4] of the modelled run: what the next run of the class is fitted to"""
    return max([r["ratio"] for r in res if r["lowered"]] + [0])


def totals(res):
    """-> (scores, counters[0], counters[7]) of the modelled run"""
    return [r["score"] for r in res], sum(r["adv2p"] for r in res), sum(r["miss"] for r in res)


def native_fit(tmp_dir):
    """qe_types.h's narrow_fit_* compiled for the host, as narrow_lib.native_rule compiles the rule"""
    return host_lib(tmp_dir, "narrow_fit",
                    'extern "C" int nf_rhat(int q, int c) { return qe::narrow_rhat(q, c); }\n'
                    'extern "C" int nf_room(int m, int n, int c1, int c) { return qe::narrow_room(m, n, c1, c); }\n'
                    'extern "C" int nf_slots(int m, int n, int c, int r) { return qe::narrow_fit_slots(m, n, c, r); }\n'
                    'extern "C" int nf_cutoff(int m, int n, int c, int s) { return qe::narrow_fit_cutoff(m, n, c, s); }\n'
                    'extern "C" int nf_lane(int m, int n, int c, int q, int s) { return qe::narrow_fit_lane(m, n, c, q, s); }\n'
                    'extern "C" int nf_ratio(int m, int n, int c, int r) { return qe::narrow_ratio(m, n, c, r); }\n')
