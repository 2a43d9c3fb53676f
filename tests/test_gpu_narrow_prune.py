"""The pruning threshold of a fitted first pass on the GPU (QE_NARROW_PRUNE): scores and statuses are the oracle's,
counters[0] is what both launches really advanced and counters[7] the tasks the second launch ran -- both exactly the model's
of tests/narrow_prune_lib.py: narrow_fit_lib's run, the first pass of every lane with a threshold walked by
tests/native/narrow_prune_cpu.cpp.  The forced cases run the one-lane kernel (masked_lib.ONE_LANE)."""
import functools
import shutil

import numpy as np
import pytest

import masked_lib as ML
import narrow_fit_lib as FL
import narrow_lib as NL
import narrow_prune_lib as PL
import oracle_lib as O
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

BW = 15


def batch_of(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs), dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs), dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1], dtype=np.int64)]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1], dtype=np.int64)]).astype(np.int64)
    return datagen.PairBatch(pp, po, pl, tp, to, tl)


def run_on(rb, sync=True):
    st = rb.run(capi.make_params(algo=2, only_score=True, bandwidth=BW), sync=sync)
    assert st >= 0, st
    if not sync:
        assert rb.fetch() >= 0
    scores, status = rb.scores()
    return scores, status, rb.counters()


def run(batch, sync=True):
    rb = capi.ResidentBatch(batch)
    try:
        return run_on(rb, sync)
    finally:
        rb.close()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """-> (a directory for the launch files, the CPU walk compiled into it)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    d = str(tmp_path_factory.mktemp("narrow_prune"))
    return d, PL.build_walk(d)


def q_of(pairs):
    return FL.learned_q(FL.fit_model(pairs, 0))


def ratio_of(distance, cutoff):
    return (1024 * distance + cutoff - 1) // cutoff


def _own_6kb():
    """192 pairs of 6 kb at 5 % (three groups; C = 900: nine slots at C / 2, seven fitted -- r^ = 298 needs a cutoff past 320), fitted and pruned to their own ratio"""
    pairs = ML.gen(192, 6000, 0.05, 8101)
    k = q_of(pairs)
    return pairs, k, k


def _median_6kb():
    """the same pairs pruned at the ratio of their median distance: about half of them end above their threshold"""
    pairs, k, _ = _own_6kb()
    d = sorted(r["score"] for r in FL.fit_model(pairs, 0))
    return pairs, k, ratio_of(d[len(d) // 2], NL.max_cutoff(6000, 6000, BW))


def _interleaved_6kb():
    """2 %, 5 % and 8 % reads of 6 kb in turn, every eighth pattern clipped by 300 bases (such a lane keeps C / 2 and has no
    threshold), fitted and pruned to the 5 % reads: lanes with and without a threshold, and misses, in the same passes"""
    sets = [ML.gen(64, 6000, e, 8110 + i) for i, e in enumerate((0.02, 0.05, 0.08))]
    pairs = [s[i] for i in range(64) for s in sets]
    pairs = [(p[300:], t) if i % 8 == 5 else (p, t) for i, (p, t) in enumerate(pairs)]
    k = q_of(sets[1])
    return pairs, k, k


def _ragged_symbols_4kb():
    """narrow_lib's ragged and N / lower-case / IUPAC pairs among plain 4 kb reads at 4 %, fitted and pruned to the plain reads:
    the general single-slot form, partial chunks and N under a threshold"""
    odd = [(p, t) for _, p, t in NL.ragged_pairs()][::3] + [(p, t) for _, p, t in NL.symbol_pairs()]
    plain = ML.gen(100, 4000, 0.04, 8120)
    for j, m in enumerate((3968, 3969, 3967, 3904)):
        plain[j] = (plain[j][0][:m], plain[j][1])
    out = []
    for i in range(max(len(odd), len(plain))):
        out += odd[i:i + 1] + plain[i:i + 1]
    k = q_of(plain[4:])
    return out, k, k


CASES = {"own_6kb": _own_6kb, "median_6kb": _median_6kb, "interleaved_6kb": _interleaved_6kb, "ragged_symbols_4kb": _ragged_symbols_4kb}


@functools.lru_cache(maxsize=None)
def case(name, work):
    """-> pairs, k, kp, the model of the run fitted to k and pruned at kp, the model of the fit alone -- computed once, shared"""
    pairs, k, kp = CASES[name]()
    d, exe = work
    memo = {}
    pruned, counts = PL.prune_model(pairs, k, kp, exe, d, memo=memo, name=name)
    return pairs, k, kp, pruned, FL.fit_model(pairs, k, memo=memo), counts


@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_forced_threshold_equals_the_model(monkeypatch, work, name, sync):
    pairs, k, kp, pruned, fit, counts = case(name, work)
    for key, v in dict(ML.ONE_LANE, QE_SCORE_NARROW="1", QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(kp)).items():
        monkeypatch.setenv(key, v)
    scores, status, cnt = run(batch_of(pairs), sync=sync)
    exp_score, exp_adv, exp_miss = FL.totals(pruned)
    fit_adv, fit_miss = FL.totals(fit)[1:]
    with_thr = sum(r["prune"] < r["cut1"] for r in pruned)
    without = sum(r["lowered"] and r["prune"] == r["cut1"] for r in pruned)
    print(name, sync, "k", k, "kp", kp, "pairs", len(pairs), "lanes with a threshold", with_thr, "lowered without", without, "misses", int(cnt[7]),
          "expected", exp_miss, "the fit alone", fit_miss, "adv", int(cnt[0]), "expected", exp_adv, "the fit alone", fit_adv, counts)
    assert scores.tolist() == exp_score
    assert (status == O.WIP).all()
    assert cnt[7] == exp_miss and cnt[0] == exp_adv
    if name == "own_6kb":
        assert exp_miss == 0 and fit_miss == 0 and with_thr == len(pairs) and exp_adv < fit_adv
        assert {NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(pairs, pruned)} == {7}
        first = sum(r["adv1"] for r in pruned)
        assert first < sum(r["adv1"] for r in fit)               # both band-edge rules fire: the first pass itself is lower
    if name == "median_6kb":
        assert fit_miss == 0 and len(pairs) // 4 < exp_miss < 3 * len(pairs) // 4
        assert exp_miss == sum(r["fit_miss"] for r in pruned)    # every one of them is owed to the threshold: stat[5]
    if name == "interleaved_6kb":
        assert with_thr > 0 and without > 0 and exp_miss >= fit_miss > 0      # (the 8 % reads miss with or without it)
        assert sum(r["prune"] < r["cut1"] and not r["miss"] for r in pruned) > 0
    if name == "ragged_symbols_4kb":
        thr_n = sum(r["prune"] < r["cut1"] and (b"N" in p or b"N" in t) for (p, t), r in zip(pairs, pruned))
        ragged = sum(r["prune"] < r["cut1"] and len(t) % 64 != 0 for (p, t), r in zip(pairs, pruned))
        assert thr_n > 0 and ragged > 0 and 0 < exp_miss < len(pairs)


@pytest.mark.parametrize("sync", [True, False])
def test_switched_off_is_the_fit_alone(monkeypatch, work, sync):
    pairs, k, _, pruned, fit, _ = case("own_6kb", work)
    for key, v in dict(ML.ONE_LANE, QE_SCORE_NARROW="1", QE_NARROW_FIT=str(k), QE_NARROW_PRUNE="0").items():
        monkeypatch.setenv(key, v)
    scores, _, cnt = run(batch_of(pairs), sync=sync)
    exp_score, exp_adv, exp_miss = FL.totals(fit)
    assert scores.tolist() == exp_score and cnt[0] == exp_adv and cnt[7] == exp_miss
    assert cnt[0] > FL.totals(pruned)[1]


@functools.lru_cache(maxsize=None)
def big_case(work):
    """a list above the default gate: 64 x 1 032 pairs of 4 kb at 5 % (C = 600: six slots at C / 2, five fitted)"""
    batch = datagen.generate(count=64 * (1024 + 8), length=4000, error=0.05, seed=8201)
    pairs = list(batch.pairs())
    d, exe = work
    memo = {}
    half = FL.fit_model(pairs, 0, memo=memo)
    q1 = FL.learned_q(half)
    fit = FL.fit_model(pairs, q1, memo=memo)
    pruned, _ = PL.prune_model(pairs, q1, PL.policy_qp([q1, FL.learned_q(fit)]), exe, d, memo=memo, name="big")
    return batch, pairs, q1, half, fit, pruned


def test_learning_at_the_default_switches(monkeypatch, work):
    """run 1 walks C / 2, run 2 the fit alone (one report in the ring: no threshold), runs 3 and 4 carry the threshold -- on one
    replayed list the two reports are equal, so it is r^ itself"""
    for key in ("QE_SCORE_NARROW", "QE_NARROW_FIT", "QE_NARROW_PRUNE"):
        monkeypatch.delenv(key, raising=False)
    capi.reload_env()
    batch, pairs, q1, half, fit, pruned = big_case(work)
    exp_score, adv1, miss1 = FL.totals(half)
    _, adv2, miss2 = FL.totals(fit)
    _, adv3, miss3 = FL.totals(pruned)
    assert q1 > 0 and FL.learned_q(fit) == q1 and FL.learned_q(pruned) == q1 and (miss1, miss2, miss3) == (0, 0, 0)
    assert adv3 < adv2 < adv1
    assert {NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(pairs, fit)} == {5}
    assert exp_score[:512] == [O.oracle_align(p, t, algo=O.BANDED, only_score=True, bandwidth=BW)[1] for p, t in pairs[:512]]
    rb = capi.ResidentBatch(batch)
    try:
        for k, (adv, sync) in enumerate(((adv1, True), (adv2, False), (adv3, True), (adv3, False))):
            scores, status, cnt = run_on(rb, sync)
            print("run", k + 1, "adv", int(cnt[0]), "expected", adv, "misses", int(cnt[7]))
            assert scores.tolist() == exp_score and (status == O.WIP).all()
            assert cnt[0] == adv and cnt[7] == 0
        monkeypatch.setenv("QE_NARROW_PRUNE", "0")
        capi.reload_env()                                        # (forgets what the class has learnt: C / 2, then the fit, and it stays)
        for k, adv in enumerate((adv1, adv2, adv2, adv2)):
            scores, status, cnt = run_on(rb, k % 2 == 0)
            print("switched off, run", k + 1, "adv", int(cnt[0]), "expected", adv)
            assert scores.tolist() == exp_score and cnt[0] == adv and cnt[7] == 0
    finally:
        rb.close()
