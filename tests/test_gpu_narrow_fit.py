"""The fitted first pass of BandEd score-only in two passes on the GPU (QE_NARROW_FIT): scores and statuses are the single
pass's, counters[0] is what both passes really advanced and counters[7] the tasks the second pass ran -- both exactly the
model's of tests/narrow_fit_lib.py: groups of 64 in library order, one slot count per group, the oracle's pass at the fitted
cutoffs, the rule of qe_types.h, the oracle's pass at C."""
import functools

import numpy as np
import pytest

import narrow_fit_lib as FL
import narrow_lib as NL
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


def gen(count, length, error, seed, **kw):
    return list(datagen.generate(count=count, length=length, error=error, seed=seed, **kw).pairs())


def q_of(pairs):
    """the ratio a run at C / 2 over these pairs reports: the oracle's scores"""
    return FL.learned_q(FL.fit_model(pairs, 0))


def _easy_3kb():
    pairs = gen(150, 3000, 0.02, 5101)
    return pairs, q_of(pairs)


def _interleaved():
    """2 %, 4 % and 12 % reads of 3 kb in turn (one length: every wave holds all three), fitted to the 2 % ones: misses owed
    to the fit alone, misses C / 2 would have had too, and accepted tasks in every group"""
    sets = [gen(64, 3000, e, 5110 + i) for i, e in enumerate((0.02, 0.04, 0.12))]
    return [s[i] for i in range(64) for s in sets], q_of(sets[0])


def _ragged_and_symbols():
    """narrow_lib's ragged and N / lower-case / IUPAC pairs, fitted to the middle one of the ratios they report at C / 2:
    half of them are too far for the fit"""
    pairs = [(p, t) for _, p, t in NL.ragged_pairs()][::3] + [(p, t) for _, p, t in NL.symbol_pairs()]
    seen = sorted(r["ratio"] for r in FL.fit_model(pairs, 0) if r["ratio"] > 0)
    return pairs, seen[len(seen) // 2]


def _floor():
    return gen(100, 200, 0.05, 5120), 400                  # both bands are the floor's: nothing to fit


def _indel_10kb():
    """two 500-base indels per pair: |m - n| differs from lane to lane, so the groups' slot counts are those of their neediest
    lanes and some lanes keep C / 2"""
    return gen(70, 10000, 0.05, 5130, indels_num=2, indels_len=500), q_of(gen(16, 10000, 0.05, 5131))


CASES = {"easy_3kb": _easy_3kb, "interleaved": _interleaved, "ragged_symbols": _ragged_and_symbols, "floor": _floor,
         "indel_10kb": _indel_10kb}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> pairs, k, the model of the run fitted to k, the model at C / 2 -- computed once, shared by the tests, never changed"""
    pairs, k = CASES[name]()
    memo = {}
    return pairs, k, FL.fit_model(pairs, k, memo=memo), FL.fit_model(pairs, 0, memo=memo)


@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_forced_fit_equals_the_model(monkeypatch, name, sync):
    pairs, k, fit, half = case(name)
    monkeypatch.setenv("QE_SCORE_NARROW", "1")
    monkeypatch.setenv("QE_NARROW_FIT", str(k))
    scores, status, cnt = run(batch_of(pairs), sync=sync)
    exp_score, exp_adv, exp_miss = FL.totals(fit)
    fitted = sum(a["cut1"] != b["cut1"] for a, b in zip(fit, half))
    print(name, sync, "k", k, "pairs", len(pairs), "fitted", fitted, "misses", int(cnt[7]), "expected", exp_miss,
          "of them the fit's", sum(r["fit_miss"] for r in fit), "adv", int(cnt[0]), "expected", exp_adv, "at C / 2", FL.totals(half)[1])
    assert scores.tolist() == exp_score
    assert (status == O.WIP).all()
    assert cnt[7] == exp_miss and cnt[0] == exp_adv
    slots = lambda res: {NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(pairs, res)}
    if name == "easy_3kb":
        assert exp_miss == 0 and slots(half) == {5} and slots(fit) == {3}
    if name == "interleaved":
        own = sum(r["fit_miss"] for r in fit)
        assert own > 0 and exp_miss - own > 0 and sum(r["lowered"] and not r["miss"] for r in fit) > 0
    if name == "ragged_symbols":
        assert 0 < exp_miss < len(pairs) and fitted > 0
    if name == "floor":
        assert fitted == 0 and (exp_adv, exp_miss) == FL.totals(half)[1:]
        res = NL.two_pass_many(pairs, bandwidth=BW)
        assert exp_adv == sum(r["adv2p"] for r in res) and not any(r["narrower"] for r in res)
    if name == "indel_10kb":
        assert 0 < fitted < sum(r["lowered"] for r in fit)


@pytest.mark.parametrize("sync", [True, False])
def test_switched_off_is_half_the_cutoff(monkeypatch, sync):
    pairs, _, fit, _ = case("easy_3kb")
    monkeypatch.setenv("QE_SCORE_NARROW", "1")
    monkeypatch.setenv("QE_NARROW_FIT", "0")
    scores, _, cnt = run(batch_of(pairs), sync=sync)
    res = NL.two_pass_many(pairs, bandwidth=BW)
    assert scores.tolist() == [r["score"] for r in res]
    assert cnt[0] == sum(r["adv2p"] for r in res) and cnt[7] == sum(r["miss"] for r in res)
    assert cnt[0] > FL.totals(fit)[1]


def big_list(length, error, seed):
    """a list above the default gate (one group of 64 per SIMD): 1 032 groups, eight more than a 256-CU device has SIMDs"""
    return datagen.generate(count=64 * (1024 + 8), length=length, error=error, seed=seed)


def test_learning_at_the_default_switches(monkeypatch):
    """2 kb reads at 2 %: unknown data take C / 2 (four slots of the six at C = 300), the runs after it the three slots that
    prove what run 1 saw.  Then 4 % reads of the same length class under the stale fit: that run's second-pass tasks are the
    model's (three slots are this class's floor and their roomiest cutoff, 128, still proves these distances, so the model has
    none; a stale fit that does miss is the forced "interleaved" case above and tests/native/narrow_fit_host.cpp), it reports
    their ratios, and the runs after it are fitted to those -- the class never falls to the single pass"""
    monkeypatch.delenv("QE_SCORE_NARROW", raising=False)
    monkeypatch.delenv("QE_NARROW_FIT", raising=False)
    capi.reload_env()
    easy, hard = big_list(2000, 0.02, 5201), big_list(2000, 0.04, 5202)
    ep, hp = list(easy.pairs()), list(hard.pairs())
    memo = {}
    first = FL.fit_model(ep, 0, memo=memo)
    res = NL.two_pass_many(ep[:2048], bandwidth=BW)                      # (q = 0 IS narrow_lib's model)
    assert [r["adv2p"] for r in first[:2048]] == [r["adv2p"] for r in res]
    q1 = FL.learned_q(first)
    fit = FL.fit_model(ep, q1, memo=memo)
    exp_score, adv1, miss1 = FL.totals(first)
    _, adv2, miss2 = FL.totals(fit)
    assert q1 > 0 and miss1 == 0 and miss2 == 0 and adv2 < adv1 and FL.learned_q(fit) == q1
    rb = capi.ResidentBatch(easy)
    try:
        for k, (adv, sync) in enumerate(((adv1, True), (adv2, False), (adv2, True))):
            scores, status, cnt = run_on(rb, sync)
            print("easy run", k + 1, "adv", int(cnt[0]), "expected", adv, "misses", int(cnt[7]))
            assert scores.tolist() == exp_score and (status == O.WIP).all()
            assert cnt[0] == adv and cnt[7] == 0
    finally:
        rb.close()
    memo = {}
    stale = FL.fit_model(hp, q1, memo=memo)
    q2 = max(q1, FL.learned_q(stale))
    refit = FL.fit_model(hp, q2, memo=memo)
    hard_score, adv3, miss3 = FL.totals(stale)
    _, adv4, miss4 = FL.totals(refit)
    print("hard list: q", q1, "->", q2, "misses of the stale fit", miss3, "of them the fit's own", sum(r["fit_miss"] for r in stale))
    assert miss3 == sum(r["fit_miss"] for r in stale) and q2 > q1 and miss4 == 0      # (no miss half the cutoff would have had too)
    rb = capi.ResidentBatch(hard)
    try:
        for k, (adv, miss, sync) in enumerate(((adv3, miss3, False), (adv4, 0, True), (adv4, 0, False))):
            scores, status, cnt = run_on(rb, sync)
            print("hard run", k + 1, "adv", int(cnt[0]), "expected", adv, "misses", int(cnt[7]), "expected", miss)
            assert scores.tolist() == hard_score and (status == O.WIP).all()
            assert cnt[0] == adv and cnt[7] == miss
    finally:
        rb.close()
