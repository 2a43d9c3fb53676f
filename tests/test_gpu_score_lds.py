"""Band state in LDS for the first launch of a two-pass BandEd score-only run (QE_SCORE_LDS): k_banded<false, true>
keeps Pv, Mv and the scores ring of every wave in its slice of the workgroup's LDS.  Every case runs the one-lane kernel
(masked_lib.ONE_LANE) under QE_SCORE_NARROW=1 and a forced QE_NARROW_FIT, with and without a forced QE_NARROW_PRUNE, once with
QE_SCORE_LDS=1 and once with 0: scores, statuses and counters[0] / [7] are identical between the two and equal to the model
of tests/narrow_prune_lib.py (the oracle's passes; lanes with a threshold walked by tests/native/narrow_prune_cpu.cpp).
Which form the first launch took is read from the library's QE_TRACE line."""
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
    d = str(tmp_path_factory.mktemp("score_lds"))
    return d, PL.build_walk(d)


def q_of(pairs):
    return FL.learned_q(FL.fit_model(pairs, 0))


def _partial_groups():
    """290 pairs = five groups, the last one of 34 lanes (a workgroup of four waves and one of a single wave, each wave with
    its own slice), 1.2-3 kb at 2-6 %: bands of three to five slots, one slice size for all"""
    sets = [ML.gen(58, length, e, 8300 + i) for i, (length, e) in enumerate(((1200, 0.02), (1700, 0.03), (2200, 0.04), (2600, 0.05), (3000, 0.06)))]
    pairs = [p for s in sets for p in s]
    return pairs, q_of(pairs), {}


def _ring_wrap():
    """patterns of 38-45 block rows (the ring of 16 wraps more than twice) against texts longer and shorter than the pattern by
    up to the band at half the cutoff: bands that run past row nw - 1 and bands that stop short of it, lanes that differ
    in m - n in every group"""
    base = ML.gen(150, 2880, 0.03, 8310)
    out = []
    for i, (p, t) in enumerate(base):
        d = (i * 37) % 200
        if i % 3 == 0:
            out.append((p[:len(p) - d], t))              # text longer: the band runs past row nw - 1
        elif i % 3 == 1:
            out.append((p, t[:len(t) - d]))              # text shorter: the band stops short of it
        else:
            out.append((p, t))
    return out, q_of(base), {}


def _ring_wrap_union():
    pairs, k, _ = _ring_wrap()
    return pairs, k, {"QE_LANE_REL": "0"}


def _edge(length):
    pairs = ML.gen(70, length, 0.05, 8320)
    return pairs, 1000, {}             # a ratio no narrower band proves: every lane keeps C / 2, the launch walks its bound


def _general_passes():
    """narrow_lib's ragged pairs and its N / lower-case / IUPAC pairs among plain 4 kb reads at 4 %, four of them with patterns
    whose last block row is partial, full or one base: the general single-slot passes on LDS state"""
    odd = [(p, t) for _, p, t in NL.ragged_pairs()][::3] + [(p, t) for _, p, t in NL.symbol_pairs()]
    plain = ML.gen(100, 4000, 0.04, 8330)
    for j, m in enumerate((3968, 3969, 3967, 3904)):
        plain[j] = (plain[j][0][:m], plain[j][1])
    out = []
    for i in range(max(len(odd), len(plain))):
        out += odd[i:i + 1] + plain[i:i + 1]
    return out, q_of(plain[4:]), {}


def _handover():
    """2 %, 5 % and 8 % reads of 6 kb in turn, fitted to the 2 % ones: the others miss, their second launch is the global
    form at the full cutoff (16 slots: no slice holds it)"""
    sets = [ML.gen(64, 6000, e, 8340 + i) for i, e in enumerate((0.02, 0.05, 0.08))]
    return [s[i] for i in range(64) for s in sets], q_of(sets[0]), {}


CASES = {
    "partial_groups": _partial_groups, "ring_wrap": _ring_wrap, "ring_wrap_union": _ring_wrap_union,
    "edge_cap": lambda: _edge(10000), "edge_cap_plus_1": lambda: _edge(10300),
    "general_passes": _general_passes, "handover": _handover,
}


@functools.lru_cache(maxsize=None)
def case(name, prune, work):
    """-> pairs, switches, k, kp, the model's (scores, counters[0], counters[7]) -- computed once, shared, never changed"""
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
def test_lds_form_equals_the_global_form_and_the_oracle(monkeypatch, capfd, work, name, prune):
    pairs, env, k, kp, model = case(name, prune, work)
    exp = FL.totals(model)
    bound = bound_of(pairs)
    for key, v in dict(ML.ONE_LANE, QE_SCORE_NARROW="1", QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(kp), QE_TRACE="1", **env).items():
        monkeypatch.setenv(key, v)
    batch = batch_of(pairs)
    seen = {}
    for lds in ("1", "0"):
        monkeypatch.setenv("QE_SCORE_LDS", lds)
        capfd.readouterr()
        scores, status, cnt = run(batch)
        err = capfd.readouterr().err
        form = re.findall(r"first launch of (\d+) groups, band state in (LDS|the group workspace) \((\d+) slots\)", err)
        with capfd.disabled():
            print(name, "prune", kp, "QE_SCORE_LDS", lds, "bound", bound, form, "adv / second-pass tasks", cnt, "expected", exp[1:])
        assert len(form) == 1, err[-2000:]
        if lds == "1" and bound <= CAP:
            assert form[0] == (str((len(pairs) + 63) // 64), "LDS", str(bound))
        else:
            assert form[0][1:] == ("the group workspace", "0")
        assert scores == exp[0], (name, lds)
        assert status == [O.WIP] * len(pairs), (name, lds)
        assert cnt == (exp[1], exp[2]), (name, lds)
        seen[lds] = (scores, status, cnt)
    assert seen["1"] == seen["0"]
    slots = {NL.slots(len(p), len(t), r["cut1"]) for (p, t), r in zip(pairs, model)}
    if name == "edge_cap":
        assert bound == CAP and slots == {CAP}              # all 13 slots of the slice are walked
    if name == "edge_cap_plus_1":
        assert bound == CAP + 1
    if name == "partial_groups":
        assert len(pairs) == 290 and len(slots) > 1
    if name.startswith("ring_wrap"):
        nw = [(len(p) + 63) // 64 for p, _ in pairs]
        assert min(nw) >= 36 and {-1, 1} <= {int(np.sign(len(p) - len(t))) for p, t in pairs}
        assert len({len(p) - len(t) for p, t in pairs[:64]}) > 8
    if name == "general_passes":
        assert any(b"N" in p or b"N" in t for p, t in pairs) and any(len(p) % 64 and len(t) % 64 for p, t in pairs)
    if name == "handover":
        assert len(pairs) // 3 <= exp[2] < len(pairs) and bound <= CAP
        assert max(NL.slots(len(p), len(t), NL.max_cutoff(len(p), len(t), BW)) for p, t in pairs) > CAP
