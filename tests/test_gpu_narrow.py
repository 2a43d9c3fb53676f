"""BandEd score-only in two passes on the GPU (QE_SCORE_NARROW): scores and statuses are the single pass's -- the oracle's,
the golden sets' -- while counters[0] is what both passes really advanced and counters[7] the tasks the second pass ran.
The expected figures come from tests/narrow_lib.py (the oracle's pass at C / 2, the rule of qe_types.h, its pass at C)."""
import numpy as np
import pytest

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


def run(batch, sync=True, bandwidth=BW):
    rb = capi.ResidentBatch(batch)
    st = rb.run(capi.make_params(algo=2, only_score=True, bandwidth=bandwidth), sync=sync)
    assert st >= 0, st
    if not sync:
        assert rb.fetch() >= 0
    scores, status = rb.scores()
    cnt = rb.counters()
    rb.close()
    return scores, status, cnt


def expect(pairs, bandwidth=BW):
    res = NL.two_pass_many(pairs, bandwidth=bandwidth)
    return ([r["score"] for r in res], sum(r["adv2p"] for r in res), sum(r["miss"] for r in res), sum(r["adv"] for r in res), res)


def mixed_pairs():
    """3 kb reads at 3 % (accepted), 12 % (missed) and 7.4 % (either) in turn: the library sorts by length, which these share,
    so every wave holds all three kinds; then the ragged and the N / lower-case / IUPAC pairs of the CPU grid"""
    sets = [list(datagen.generate(count=90, length=3000, error=e, seed=4100 + i).pairs()) for i, e in enumerate((0.03, 0.12, 0.074))]
    pairs = [s[i] for i in range(90) for s in sets]
    pairs += [(p, t) for _, p, t in NL.ragged_pairs()][::3]
    pairs += [(p, t) for _, p, t in NL.symbol_pairs()]
    return pairs


CASES = {
    "mixed": mixed_pairs,
    "all_miss": lambda: list(datagen.generate(count=150, length=3000, error=0.12, seed=4201).pairs()),
    "none_miss": lambda: list(datagen.generate(count=150, length=3000, error=0.03, seed=4202).pairs()),
    "floor": lambda: list(datagen.generate(count=100, length=200, error=0.05, seed=4203).pairs()),     # both bands are the floor's
    "indel_10kb": lambda: list(datagen.generate(count=70, length=10000, error=0.05, seed=4204, indels_num=2, indels_len=500).pairs()),
}


@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_forced_two_passes_equal_the_oracle(monkeypatch, name, sync):
    monkeypatch.setenv("QE_SCORE_NARROW", "1")
    pairs = CASES[name]()
    scores, status, cnt = run(batch_of(pairs), sync=sync)
    exp_score, exp_adv, exp_miss, _, res = expect(pairs)
    print(name, sync, "pairs", len(pairs), "misses", int(cnt[7]), "expected", exp_miss, "adv", int(cnt[0]), "expected", exp_adv)
    assert scores.tolist() == exp_score
    assert (status == O.WIP).all()
    assert cnt[7] == exp_miss and cnt[0] == exp_adv
    if name == "all_miss":
        assert exp_miss == len(pairs)
    if name == "none_miss":
        assert exp_miss == 0
    if name == "mixed":
        assert 0 < exp_miss < len(pairs)
    if name == "floor":
        assert not any(r["narrower"] for r in res)


def test_forced_two_passes_on_the_golden_sets(monkeypatch, golden):
    monkeypatch.setenv("QE_SCORE_NARROW", "1")
    for name, entry in golden["datasets"].items():
        if entry["gen"]["length"] > 10000:
            continue
        batch = datagen.generate(**entry["gen"])
        for label, r in entry["runs"].items():
            p = r["params"]
            if p.get("algo") != 2 or not p.get("only_score"):
                continue
            scores, status, cnt = run(batch, bandwidth=p["bandwidth"])
            assert status.tolist() == r["status"], (name, label)
            assert scores.tolist() == r["score"], (name, label)
            _, exp_adv, exp_miss, _, _ = expect(list(batch.pairs()), bandwidth=p["bandwidth"])
            assert cnt[0] == exp_adv and cnt[7] == exp_miss, (name, label)


@pytest.mark.parametrize("sync", [True, False])
def test_switched_off_is_the_single_pass(monkeypatch, sync):
    monkeypatch.setenv("QE_SCORE_NARROW", "0")
    pairs = mixed_pairs()
    scores, status, cnt = run(batch_of(pairs), sync=sync)
    exp_score, _, _, exp_single, _ = expect(pairs)
    assert scores.tolist() == exp_score and cnt[0] == exp_single and cnt[7] == 0


def big_list(length, error, seed):
    """a list above the default gate (one group of 64 per SIMD): 1 032 groups, eight more than a 256-CU device has SIMDs"""
    return datagen.generate(count=64 * (1024 + 8), length=length, error=error, seed=seed)


@pytest.mark.parametrize("sync", [True, False])
def test_default_switch_above_the_gate(monkeypatch, sync):
    """1 kb reads at 5 %: four slots at C = 150, three at C' = 75; unknown data take the first pass, and a run without misses
    has paid, so every run of this stream is a two-pass run"""
    monkeypatch.delenv("QE_SCORE_NARROW", raising=False)
    batch = big_list(1000, 0.05, 4301)
    pairs = list(batch.pairs())
    exp_score, exp_adv, exp_miss, exp_single, _ = expect(pairs)
    assert exp_miss == 0 and exp_adv < exp_single
    for _ in range(2):
        scores, status, cnt = run(batch, sync=sync)
        print("default switch", sync, "adv", int(cnt[0]), "two passes", exp_adv, "single", exp_single, "misses", int(cnt[7]))
        assert scores.tolist() == exp_score and (status == O.WIP).all()
        assert cnt[0] == exp_adv and cnt[7] == exp_miss


def test_default_switch_below_the_gate_is_the_single_pass(monkeypatch):
    monkeypatch.delenv("QE_SCORE_NARROW", raising=False)
    pairs = CASES["none_miss"]()
    scores, _, cnt = run(batch_of(pairs))
    exp_score, _, _, exp_single, _ = expect(pairs)
    assert scores.tolist() == exp_score and cnt[0] == exp_single and cnt[7] == 0


def test_policy_leaves_the_first_pass_where_it_does_not_pay(monkeypatch):
    """1 100-base reads at 12 % (a length class of their own in this suite): every task misses.  The first run on unknown
    data takes the first pass and learns that; the next 15 eligible runs take the single pass, the 16th is a single pass with
    a probe beside it (every 16th group at the halved cutoff).  The scores never change, and every run's counters are one of
    the three forms', exactly.  (Setting or removing a switch has the library forget its verdicts: the test starts from
    unknown data whatever ran before it in the process.)"""
    monkeypatch.delenv("QE_SCORE_NARROW", raising=False)
    capi.reload_env()
    batch = big_list(1100, 0.12, 4302)
    pairs = list(batch.pairs())
    exp_score, exp_adv, exp_miss, exp_single, res = expect(pairs)
    assert exp_miss == len(pairs)
    probe_adv = NL.probe_expectation(pairs, res)
    assert exp_single < probe_adv < exp_adv
    forms = {(exp_adv, exp_miss): "two", (exp_single, 0): "single", (probe_adv, 0): "probe"}
    seen = []
    for k in range(18):
        scores, _, cnt = run(batch, sync=(k % 2 == 0))
        assert scores.tolist() == exp_score, k
        assert (int(cnt[0]), int(cnt[7])) in forms, (k, int(cnt[0]), int(cnt[7]), list(forms))
        seen.append(forms[(int(cnt[0]), int(cnt[7]))])
    print("runs:", seen)
    assert seen == ["two"] + ["single"] * 15 + ["probe", "single"]


def test_a_probe_that_finds_the_first_pass_paying_brings_it_back(monkeypatch):
    """the verdict "does not pay" from 12 % reads, then 3 % reads of the same length class: 15 single passes, then the probe,
    whose sample has no miss; the run after it takes both passes again"""
    monkeypatch.delenv("QE_SCORE_NARROW", raising=False)
    capi.reload_env()
    hard, easy = big_list(1100, 0.12, 4302), big_list(1100, 0.03, 4303)
    pairs = list(easy.pairs())
    exp_score, exp_adv, exp_miss, exp_single, res = expect(pairs)
    assert exp_miss == 0
    _, _, cnt = run(hard)
    assert cnt[7] == 64 * (1024 + 8)
    seen = []
    for k in range(18):
        scores, _, cnt = run(easy, sync=(k % 2 == 1))
        assert scores.tolist() == exp_score, k
        seen.append(int(cnt[0]))
    assert seen == [exp_single] * 15 + [NL.probe_expectation(pairs, res), exp_adv, exp_adv]


def test_one_long_outlier_keeps_the_single_pass(monkeypatch):
    """a uniform workspace sized for one 40 kb pair among 1 kb reads would be many times the list's own: not taken"""
    monkeypatch.setenv("QE_SCORE_NARROW", "1")
    pairs = list(datagen.generate(count=400, length=1000, error=0.05, seed=4401).pairs())
    pairs += list(datagen.generate(count=1, length=40000, error=0.05, seed=4402).pairs())
    scores, _, cnt = run(batch_of(pairs))
    exp_score, _, _, exp_single, _ = expect(pairs)
    assert scores.tolist() == exp_score and cnt[0] == exp_single and cnt[7] == 0
