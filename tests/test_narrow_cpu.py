"""BandEd score-only in two passes, the part that needs no GPU: the property the first pass rests on, checked with the
oracle.  A pass at C' = C / 2 that returns 0 <= r' <= C', in bands that hold every diagonal a path of cost r' can touch
(narrow_lib.accepts = qe_types.h: narrow_accepts), is accepted; every accepted pair must have the score of the pass at C.
"0 <= r' <= C'" alone is NOT enough: test_the_plain_rule_has_exceptions keeps the pairs that show it.
A condition, not a measurement: zero exceptions over the grid of tests/narrow_lib.py (lengths 200 .. 10 000, error
rates on both sides of the halved cutoff, large indels, ragged lengths around C', N / lower-case / IUPAC symbols, cutoffs
around the floor of 65 and around multiples of 64)."""
import os
import re

import shutil

import pytest

import masked_lib as ML
import narrow_lib as NL
import oracle_lib as O
import unequal_lib as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(cases, cutoffs=None):
    labels = [c[0] for c in cases]
    pairs = [(c[1], c[2]) for c in cases]
    res = NL.two_pass_many(pairs, cutoffs=cutoffs)
    bad = [(lab, r) for lab, r in zip(labels, res) if r["narrower"] and r["accepted"] and r["score1"] != r["score"]]
    assert not bad, bad[:5]
    return labels, pairs, res


def test_accepted_first_pass_equals_the_pass_at_the_full_cutoff():
    cases = list(NL.grid_pairs())
    assert len(cases) == 3312
    labels, pairs, res = _check(cases)
    narrower = [r for r in res if r["narrower"]]
    accepted = [r for r in narrower if r["accepted"]]
    # the grid is there to exercise both outcomes: accepted pairs, and pairs the first pass proves nothing about
    assert len(accepted) > 1000 and len(narrower) - len(accepted) > 500
    # ... and up to 3 kb an accepted score is the exact distance
    ora = O.oracle()
    for (length, _, _, _), (p, t), r in zip(labels, pairs, res):
        if length <= 3000 and r["narrower"] and r["accepted"]:
            assert r["score1"] == ora.qo_exact_distance(p, len(p), t, len(t)), (length, len(p), len(t))


def test_ragged_lengths_around_the_halved_cutoff():
    _, _, res = _check(list(NL.ragged_pairs()))
    assert any(r["narrower"] and r["accepted"] for r in res) and any(r["miss"] for r in res)


def test_n_lower_case_and_iupac_symbols():
    _, _, res = _check(list(NL.symbol_pairs()))
    assert any(r["narrower"] and r["accepted"] for r in res) and any(r["miss"] for r in res)


def test_cutoffs_around_the_floor_and_multiples_of_64():
    cases = list(NL.floor_cutoffs())
    _, _, res = _check([c[:3] for c in cases], cutoffs=[c[3] for c in cases])
    assert any(not r["narrower"] for r in res)          # (a band of three slots at C has no narrower one: the floor)
    assert any(r["narrower"] and r["accepted"] for r in res)


def test_random_shapes_and_cutoffs():
    cases = list(NL.random_shapes(seed=1, rounds=200))
    _, _, res = _check([(i, p, t) for i, (p, t, _) in enumerate(cases)], cutoffs=[c for _, _, c in cases])
    assert sum(r["narrower"] and r["accepted"] for r in res) > 2000 and sum(r["miss"] for r in res) > 300


def test_the_plain_rule_has_exceptions():
    """cutoff 254 -> 127 on a pair with m - n = -3: three slots, two of them prolog, so in the last column of a chunk the band
    ends ON the main diagonal; the first pass returns 41 <= 127 for a distance of 29, which the pass at 254 finds.  The rule
    with the band's cover rejects it"""
    cases = list(NL.floor_cutoffs())
    wrong = 0
    for lab, p, t, c in cases:
        r = NL.two_pass(p, t, c)
        if r["narrower"] and 0 <= r["score1"] <= r["cut1"] and r["score1"] != r["score"]:
            wrong += 1
            assert r["miss"]
    assert wrong > 0


def test_a_first_result_above_the_halved_cutoff_is_not_accepted():
    """the rule is 0 <= r' <= C', not 'any score': a pass may return a path's cost above its cutoff"""
    seen = 0
    for _, p, t in NL.grid_pairs():
        if len(t) != 1000:
            continue
        r = NL.two_pass(p, t, NL.max_cutoff(len(p), len(t), 15))
        if r["narrower"] and r["score1"] > r["cut1"]:
            assert r["miss"]
            seen += 1
    assert seen > 0


def test_the_library_rule_is_the_modelled_rule(tmp_path):
    """qe_types.h's functions, compiled for the host, against narrow_lib's restatement on the random shapes and cutoffs and on
    every result 0 .. C' + 1 of a few of them (the CPU property above is checked on the restatement)"""
    lib = NL.native_rule(str(tmp_path))
    n = 0
    for p, t, c in NL.random_shapes(seed=2, rounds=120):
        m, nn = len(p), len(t)
        c1 = NL.narrow_cutoff(m, nn, c)
        assert lib.nr_cutoff(m, nn, c) == c1
        for cc in (c, c // 2):
            assert lib.nr_slots(m, nn, cc) == NL.slots(m, nn, cc) and lib.nr_cover(m, nn, cc) == NL.cover(m, nn, cc)
        rs = range(-1, c1 + 2) if n % 40 == 0 else (-1, 0, abs(m - nn), (abs(m - nn) + c1) // 2, c1 - 1, c1, c1 + 1)
        for r in rs:
            assert bool(lib.nr_accepts(m, nn, c1, c, r)) == NL.accepts(m, nn, c1, c, r), (m, nn, c1, c, r)
        n += 1
    assert n > 1000
    with open(os.path.join(ROOT, "quicked_amd", "csrc", "qe_pool.h")) as f:
        assert '"QE_SCORE_NARROW", -1' in f.read()


@pytest.mark.parametrize("bandwidth", [15, 40, 100])
def test_the_walk_model_holds_on_unequal_lengths(tmp_path, bandwidth):
    """tests/native/banded_walk.h (the CPU model of k_banded<false> that the GPU tests of the two-pass path compare with)
    on the grid of tests/unequal_lib.py -- texts from half to twice their pattern, where the prologue, the relative cutoff and
    the last block's place in the band take values that datagen's pairs never give them: groups of 64 in library order at
    the full cutoff and at half of it, the union walk and the lane-relative one, with and without masked passes.  Per pair
    the walk's score, first / last / pos_v and block advances are the oracle's own pass's (pass_plan_cpu: diffs), the -1
    of a band below the distance included; and the oracle's pass is the one test_oracle_vs_ref.py pins to the reference."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    exe = ML.build_walk(str(tmp_path))
    pairs = U.pairs()
    assert len(pairs) == 144 and {-1, 1} == {(len(p) > len(t)) - (len(p) < len(t)) for p, t in pairs}
    order = NL.library_order(pairs)
    full = [NL.max_cutoff(len(p), len(t), bandwidth) for p, t in pairs]
    for label, cut in (("full", full), ("half", [c // 2 for c in full])):
        path = os.path.join(str(tmp_path), f"unequal_{bandwidth}_{label}.bin")
        ML.write_launch(path, pairs, [(i, cut[i]) for i in order])
        for lane_rel in (1, 0):
            for masked in (1, 0):
                counts, code, out = ML.walk(exe, path, lane_rel, masked)
                print("unequal", bandwidth, label, "lane_rel", lane_rel, out.strip().splitlines()[0])
                assert code == 0 and counts["pairs"] == 144 and counts["diffs"] == 0 and counts["rule_diffs"] == 0, out[-2000:]
    # the pass the walk was compared with is the one behind the oracle's BANDED score-only result
    for (p, t), c in zip(pairs, full):
        assert NL.banded_score(p, t, c)[0] == O.oracle_align(p, t, algo=2, only_score=True, bandwidth=bandwidth)[1]
