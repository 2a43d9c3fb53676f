"""The fitted first pass of BandEd score-only in two passes (QE_NARROW_FIT), the part that needs no GPU.  The property the
fit rests on: a first pass at ANY cutoff c1 in 1 .. C whose result narrow_lib.accepts takes (= qe_types.h: narrow_accepts)
has the score of the pass at C -- a condition with zero exceptions, not a measurement.  Then the fit's functions against a
brute force over every cutoff, the header's functions against their restatement in tests/narrow_fit_lib.py, and the model of
a run in groups of 64 on the headline's shape."""
import numpy as np

import narrow_fit_lib as FL
import narrow_lib as NL
from quicked_amd import datagen

QS = (90, 200, 340, 520)            # ratios the fitted cutoffs are taken at: distances of 9 .. 51 % of the cutoff


def _cases():
    """(pattern, text, cutoff): narrow_lib's random shapes, ragged, symbol and floor-cutoff sets"""
    out = [(p, t, c) for p, t, c in NL.random_shapes(seed=3, rounds=150)]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.ragged_pairs()]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.symbol_pairs()]
    out += [(p, t, c) for _, p, t, c in NL.floor_cutoffs()]
    return out


def _fitted(m, n, c, q):
    """the cutoff a lane alone in its group takes at the ratio q"""
    return FL.fit_lane(m, n, c, q, FL.fit_slots(m, n, c, FL.rhat(q, c)))


def test_any_accepted_first_pass_equals_the_pass_at_the_full_cutoff():
    cases = _cases()
    rng = np.random.default_rng(31)
    full, seen = {}, set()
    accepted = rejected = 0
    for k, (p, t, c) in enumerate(cases):
        m, n = len(p), len(t)
        full[k] = NL.banded_score(p, t, c)[0]
        for c1 in [int(rng.integers(1, c + 1))] + [_fitted(m, n, c, q) for q in QS]:
            if (k, c1) in seen:
                continue
            seen.add((k, c1))
            s1 = NL.banded_score(p, t, c1)[0]
            if NL.accepts(m, n, c1, c, s1):
                accepted += 1
                assert s1 == full[k], (m, n, c, c1, s1, full[k])
            else:
                rejected += 1
    print("accepted", accepted, "rejected", rejected)
    assert accepted >= 1000 and rejected >= 300


def test_fit_functions_against_brute_force():
    cases = _cases()
    rng = np.random.default_rng(32)
    checked = fitted = 0
    for k, (p, t, c) in enumerate(cases):
        if k % 9:
            continue
        m, n = len(p), len(t)
        rows, most, where = FL.brute_force(m, n, c)
        for r_hat in {FL.rhat(q, c) for q in QS} | {int(rng.integers(0, c + 1)), abs(m - n)}:
            least = FL.brute_least_slots(m, n, c, rows, r_hat)
            s = FL.fit_slots(m, n, c, r_hat)
            assert s == least, (m, n, c, r_hat, s, least)
            checked += 1
            if least:
                c1 = FL.fit_cutoff(m, n, c, s)
                assert NL.slots(m, n, c1) == s and c1 == where[s] and FL.room(m, n, c1, c) == most[s], (m, n, c, r_hat, s, c1)
                assert NL.accepts(m, n, c1, c, r_hat)                # whenever any cutoff of fewer slots than C's does
                fitted += 1
        for s, c1 in where.items():                                  # every slot count: the roomiest cutoff, the smallest such
            assert FL.fit_cutoff(m, n, c, s) == c1 and FL.room(m, n, c1, c) == most[s], (m, n, c, s)
    print("checked", checked, "with a fit", fitted)
    assert checked > 1000 and fitted > 300


def test_the_library_fit_is_the_modelled_fit(tmp_path):
    lib = FL.native_fit(str(tmp_path))
    rng = np.random.default_rng(33)
    cnt = 0
    for p, t, c in _cases():
        m, n = len(p), len(t)
        for q in QS + (int(rng.integers(1, 1025)),):
            rh = FL.rhat(q, c)
            assert lib.nf_rhat(q, c) == rh
            s = FL.fit_slots(m, n, c, rh)
            assert lib.nf_slots(m, n, c, rh) == s, (m, n, c, rh)
            for sg in {s, s + 1, 0, 3, int(rng.integers(2, NL.slots(m, n, c) + 2))}:
                assert lib.nf_cutoff(m, n, c, sg) == FL.fit_cutoff(m, n, c, sg), (m, n, c, sg)
                assert lib.nf_lane(m, n, c, q, sg) == FL.fit_lane(m, n, c, q, sg), (m, n, c, q, sg)
            for c1 in (rh, c // 2, int(rng.integers(1, c + 1))):
                assert lib.nf_room(m, n, c1, c) == FL.room(m, n, c1, c), (m, n, c1, c)
            for r in (-1, 0, abs(m - n), rh, c // 2, c // 2 + 1, c):
                assert lib.nf_ratio(m, n, c, r) == FL.ratio(m, n, c, r), (m, n, c, r)
            cnt += 1
    assert cnt > 10000


def test_a_fit_is_lower_than_half_the_cutoff_or_is_half_the_cutoff():
    """the group rule: a lane takes the fitted cutoff only where its band has fewer slots than the band at C / 2 and proves the
    lane's own r_hat; q = 0 is C / 2 exactly"""
    for p, t, c in _cases():
        m, n = len(p), len(t)
        half = NL.narrow_cutoff(m, n, c)
        assert FL.group_cutoffs([(m, n, c)], 0) == [half]
        for q in QS:
            for sg in range(0, NL.slots(m, n, c) + 1):
                c1 = FL.fit_lane(m, n, c, q, sg)
                if c1 != half:
                    assert NL.slots(m, n, c1) == sg < NL.slots(m, n, half) and NL.accepts(m, n, c1, c, FL.rhat(q, c))


def _group_model(length, error, seeds, n=256):
    a, b = [list(datagen.generate(count=n, length=length, error=error, seed=s).pairs()) for s in seeds]
    out = []
    for mine, other in ((a, b), (b, a)):
        q = FL.learned_q(FL.fit_model(other, 0))                     # what a run at C / 2 over the OTHER sample reports
        base, fit = FL.fit_model(mine, 0), FL.fit_model(mine, q)
        assert q > 0 and all(r["lowered"] for r in base)
        assert not any(r["miss"] for r in fit) and not any(r["miss"] for r in base)
        assert [r["score1"] for r in fit] == [r["score"] for r in fit]
        slots = sorted({NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(mine, fit)})
        frac = sum(r["adv1"] for r in fit) / sum(r["adv1"] for r in base)
        print(length, error, "q", q, "slots", slots, "first-pass block-columns against C / 2: %.3f" % frac)
        out.append(frac)
    return out


def test_group_model_on_the_headline_shape():
    """256 pairs of 10 kb at 5 % in library order, groups of 64, q learnt from a sample of another seed: no miss, no wrong
    score, and the first pass advances at most 0.70 of the block-columns of the pass at C / 2"""
    for frac in _group_model(10000, 0.05, (7101, 7102)):
        assert frac <= 0.70


def test_group_model_on_3kb_at_2_percent():
    """five slots at C / 2, three fitted: 0.60 by slots, and 0.05 for the band edges, which cut a narrower band less (the
    headline's bound leaves the same share over its slot ratio)"""
    for frac in _group_model(3000, 0.02, (7103, 7104)):
        assert frac <= 0.65
