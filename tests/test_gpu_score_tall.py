"""Tall passes of k_banded<false, true> (QE_SCORE_TALL): the first launch of a two-pass BandEd score-only run with
its band state in LDS walks a chunk in one pass of 5 .. 10 slots where the plan allows it.  Every case runs the one-lane
kernel (masked_lib.ONE_LANE) under QE_SCORE_NARROW=1, a forced QE_NARROW_FIT, with and without a forced QE_NARROW_PRUNE, and
QE_SCORE_LDS=1, once with QE_SCORE_TALL=1 and once with 0: scores, statuses and counters[0] / [7] are identical between the
two and equal to the model of tests/narrow_prune_lib.py (the oracle's passes; lanes with a threshold walked by
tests/native/narrow_prune_cpu.cpp).  Which form ran is read from the library's QE_TRACE line.  What the plan does with each
of these inputs -- which heights it takes, where it falls back -- is tests/test_tall_passes_cpu.py's."""
import functools
import re
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
CAP = 13            # qe_types.h: score_lds_cap()
# (a): read length -> the slot count of its fitted first launch (70 pairs at 5 %, fitted to themselves); together 5 .. 10
HEIGHTS = {4000: 5, 5000: 6, 6000: 7, 7000: 8, 8000: 9, 10000: 10}
assert sorted(HEIGHTS.values()) == [5, 6, 7, 8, 9, 10]


def batch_of(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs), dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs), dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1], dtype=np.int64)]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1], dtype=np.int64)]).astype(np.int64)
    return datagen.PairBatch(pp, po, pl, tp, to, tl)


def run(batch):
    rb = capi.ResidentBatch(batch)
    try:
        st = rb.run(capi.make_params(algo=2, only_score=True, bandwidth=BW), sync=True)
        assert st >= 0, st
        scores, status = rb.scores()
        cnt = rb.counters()
        return scores.tolist(), status.tolist(), (int(cnt[0]), int(cnt[7]))
    finally:
        rb.close()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    d = str(tmp_path_factory.mktemp("score_tall"))
    return d, PL.build_walk(d)


def q_of(pairs):
    return FL.learned_q(FL.fit_model(pairs, 0))


def _height(length):
    """(a) 70 pairs of one length at 5 %, fitted to themselves: a group of 64 lanes and one of 6"""
    pairs = ML.gen(70, length, 0.05, 8400 + length // 1000)
    return pairs, q_of(pairs), {}


def _ragged_wave():
    """(b) 40 reads of 6 kb at 5 % and 250 of 1.2-3 kb at 2-6 %: the library orders by length, so the first wave holds the 6 kb
    reads beside 24 of the 3 kb ones -- lanes of 3-5 and of 7-8 slots in one pass, dead suffixes in a tall pass -- and the
    last of the five groups has 34 lanes"""
    sets = [ML.gen(50, length, e, 8410 + i) for i, (length, e) in enumerate(((1200, 0.02), (1700, 0.03), (2200, 0.04), (2600, 0.05), (3000, 0.06)))]
    pairs = ML.gen(40, 6000, 0.05, 8416) + [p for s in sets for p in s]
    return pairs, q_of(pairs), {}


def _ragged_wave_union():
    """(c) the same, the wave walking the union of its lanes' bands: a band that starts inside a pass sends the wave back"""
    pairs, k, _ = _ragged_wave()
    return pairs, k, {"QE_LANE_REL": "0"}


def _general_passes():
    """(d) narrow_lib's ragged pairs and its N / lower-case / IUPAC pairs among plain 4 kb reads at 4 %, four of them with
    patterns whose last block row is partial, full or one base: every one of these must leave the tall pass"""
    odd = [(p, t) for _, p, t in NL.ragged_pairs()][::3] + [(p, t) for _, p, t in NL.symbol_pairs()]
    plain = ML.gen(100, 4000, 0.04, 8330)
    for j, m in enumerate((3968, 3969, 3967, 3904)):
        plain[j] = (plain[j][0][:m], plain[j][1])
    out = []
    for i in range(max(len(odd), len(plain))):
        out += odd[i:i + 1] + plain[i:i + 1]
    return out, q_of(plain[4:]), {}


def _ring_wrap():
    """(e) patterns of 38-45 block rows against texts longer and shorter than the pattern by up to 200: bands that run past
    row nw - 1 and bands that stop short of it, lanes that differ in m - n in every group"""
    base = ML.gen(150, 2880, 0.03, 8310)
    out = []
    for i, (p, t) in enumerate(base):
        d = (i * 37) % 200
        if i % 3 == 0:
            out.append((p[:len(p) - d], t))
        elif i % 3 == 1:
            out.append((p, t[:len(t) - d]))
        else:
            out.append((p, t))
    return out, q_of(base), {}


def _edge(length):
    """(f) a ratio no narrower band proves: every lane keeps C / 2 and the launch walks its bound, 13 slots -- taller than the
    tallest pass, so the plan splits it"""
    return ML.gen(70, length, 0.05, 8320), 1000, {}


def _alone():
    """(g) one pair: a wave with 63 absent lanes"""
    pairs = ML.gen(1, 6000, 0.05, 8420)
    return pairs, q_of(pairs), {}


CASES = {f"height_{n // 1000}k": functools.partial(_height, n) for n in HEIGHTS}
CASES.update({
    "ragged_wave": _ragged_wave, "ragged_wave_union": _ragged_wave_union, "general_passes": _general_passes,
    "ring_wrap": _ring_wrap, "edge_cap": lambda: _edge(10000), "alone": _alone,
})


@functools.lru_cache(maxsize=None)
def case(name, prune, work):
    """-> pairs, switches, k, kp, the model's records -- computed once, shared, never changed"""
    pairs, k, env = CASES[name]()
    kp = k if prune else 0
    d, exe = work
    model, _ = PL.prune_model(pairs, k, kp, exe, d, name=f"{name}_{int(prune)}")
    return pairs, env, k, kp, model


def bound_of(pairs):
    """the largest slot count a first launch can walk (qe_stages.hip: score_lds_slots)"""
    return max(NL.slots(len(p), len(t), NL.narrow_cutoff(len(p), len(t), NL.max_cutoff(len(p), len(t), BW))) for p, t in pairs)


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_tall_passes_equal_the_old_plan_and_the_oracle(monkeypatch, capfd, work, name, prune):
    pairs, env, k, kp, model = case(name, prune, work)
    exp = FL.totals(model)
    bound = bound_of(pairs)
    assert bound <= CAP                                      # every case takes the LDS form: the form that has tall passes
    for key, v in dict(ML.ONE_LANE, QE_SCORE_NARROW="1", QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(kp), QE_SCORE_LDS="1", QE_TRACE="1", **env).items():
        monkeypatch.setenv(key, v)
    batch = batch_of(pairs)
    seen = {}
    for tall in ("1", "0"):
        monkeypatch.setenv("QE_SCORE_TALL", tall)
        capfd.readouterr()
        scores, status, cnt = run(batch)
        err = capfd.readouterr().err
        form = re.findall(r"first launch of (\d+) groups, band state in (LDS|the group workspace) \((\d+) slots\), tall passes (on|off)", err)
        with capfd.disabled():
            print(name, "prune", kp, "QE_SCORE_TALL", tall, "bound", bound, form, "adv / second-pass tasks", cnt, "expected", exp[1:])
        assert form == [(str((len(pairs) + 63) // 64), "LDS", str(bound), "on" if tall == "1" else "off")], err[-2000:]
        assert scores == exp[0], (name, tall)
        assert status == [O.WIP] * len(pairs), (name, tall)
        assert cnt == (exp[1], exp[2]), (name, tall)
        seen[tall] = (scores, status, cnt)
    assert seen["1"] == seen["0"]
    slots = {NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(pairs, model)}
    if name.startswith("height_"):
        assert len(pairs) == 70 and HEIGHTS[1000 * int(name[7:-1])] in slots       # 5 .. 10 over the six lengths
    if name.startswith("ragged_wave"):
        order = NL.library_order(pairs)
        first = {NL.slots(len(pairs[i][0]), len(pairs[i][1]), model[i]["cut1"]) for i in order[:64]}
        assert len(pairs) == 290 and len(pairs) % 64 == 34
        assert min(first) <= 5 and max(first) >= 7          # low and tall bands in the first wave
    if name == "general_passes":
        assert any(b"N" in p or b"N" in t for p, t in pairs) and any(len(p) % 64 and len(t) % 64 for p, t in pairs)
    if name == "ring_wrap":
        assert {-1, 1} <= {int(np.sign(len(p) - len(t))) for p, t in pairs}
    if name == "edge_cap":
        assert bound == CAP and slots == {CAP}              # 13 slots: a tall pass and the rest of the old plan
    if name == "alone":
        assert len(pairs) == 1
