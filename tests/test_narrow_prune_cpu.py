"""The pruning threshold of a fitted first pass (QE_NARROW_PRUNE), the part that needs no GPU.  The property
it rests on: the walk of k_banded<false> with the band geometry of c1 and the band-edge rules at a threshold p <= c1 returns,
whenever qe_types.h's narrow_accepts_pruned takes its result (narrow_accepts and r <= p), the score of the pass at the full
cutoff C -- a condition with zero exceptions.  tests/native/narrow_prune_cpu.cpp walks the passes; `pytest -s` prints the
counts and the live slots per chunk."""
import os
import shutil

import numpy as np
import pytest

import masked_lib as ML
import narrow_fit_lib as FL
import narrow_lib as NL
import narrow_prune_lib as PL

QS = (90, 200, 340, 520)            # the ratios of tests/test_narrow_fit_cpu.py
PERCENT = (15, 30, 50, 70, 90)
MASKED_CASES = ("interleaved", "indels", "ragged_symbols", "last_row", "fit_interleaved")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    return PL.build_walk(str(tmp_path_factory.mktemp("narrow_prune")))


def _cases():
    """(pattern, text, cutoff): narrow_lib's random shapes, ragged, symbol and floor-cutoff sets"""
    out = [(p, t, c) for p, t, c in NL.random_shapes(seed=3, rounds=150)]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.ragged_pairs()]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.symbol_pairs()]
    out += [(p, t, c) for _, p, t, c in NL.floor_cutoffs()]
    return out


def test_the_library_rule_is_the_modelled_rule(tmp_path):
    lib = PL.native_rule(str(tmp_path))
    rng = np.random.default_rng(41)
    cnt = 0
    for p, t, c in _cases()[::3]:
        m, n = len(p), len(t)
        for q in QS:
            c1 = FL.fit_lane(m, n, c, q, FL.fit_slots(m, n, c, FL.rhat(q, c)))
            for qp in (0, q, q + 40, 1500, int(rng.integers(1, 1025))):
                pr = PL.prune_of(m, n, c, c1, qp)
                assert lib.np_prune(m, n, c, c1, qp) == pr and pr <= c1, (m, n, c, c1, qp)
                for r in (-1, abs(m - n), pr - 1, pr, pr + 1, c1):
                    assert bool(lib.np_accepts(m, n, c1, c, pr, r)) == PL.accepts_pruned(m, n, c1, c, pr, r)
                cnt += 1
    assert cnt > 5000


def test_any_accepted_pruned_first_pass_equals_the_pass_at_the_full_cutoff(exe, tmp_path):
    """p uniform in [max(1, d - 24), c1] around the oracle's distance d (pairs beyond c1: uniform in [1, c1])"""
    cases = _cases()
    rng = np.random.default_rng(42)
    launch, dist = [], []
    for k, (p, t, c) in enumerate(cases):
        m, n = len(p), len(t)
        d = NL.banded_score(p, t, c)[0]
        for c1 in sorted({FL.fit_lane(m, n, c, q, FL.fit_slots(m, n, c, FL.rhat(q, c))) for q in QS}):
            lo = max(1, d - 24) if 0 <= d <= c1 else 1
            launch.append((k, c1, int(rng.integers(min(lo, c1), c1 + 1)), c))
            dist.append(d)
    rows, counts = PL.walk_many(exe, str(tmp_path), [(p, t) for p, t, _ in cases], launch, name="draws")
    below = sum(1 for (k, c1, p, c), d, (s, a, ok) in zip(launch, dist, rows) if 0 <= d <= c1 and p < d and not ok)
    print("draws", len(launch), counts, "rejected because p < d:", below)
    assert counts["diffs"] == 0 and counts["rule_diffs"] == 0
    assert counts["accepted"] + counts["rejected"] == len(launch)
    assert 2 * counts["accepted"] >= len(launch) and below >= 200


@pytest.mark.parametrize("lane_rel", [1, 0])
@pytest.mark.parametrize("name", MASKED_CASES)
def test_masked_cases_under_thresholds(exe, tmp_path, name, lane_rel):
    """the launches of tests/masked_lib.py at 15 .. 90 % of every task's launch cutoff: most pairs lie above the low ones"""
    pairs, _, _, launches = ML.case(name)
    full = [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in pairs]
    for k, launch in enumerate(launches):
        for pct in PERCENT:
            path = os.path.join(str(tmp_path), f"{name}_{k}_{pct}.bin")
            PL.write_launch(path, pairs, [(i, c1, max(1, c1 * pct // 100), full[i]) for i, c1 in launch])
            counts, rows, code, out = PL.walk(exe, path, lane_rel, 1)
            print(name, k, "lane_rel", lane_rel, pct, "%:", out.strip().splitlines()[0])
            assert code == 0 and counts["diffs"] == 0 and counts["rule_diffs"] == 0 and counts["lost"] == 0, out[-2000:]
            assert len(rows) == len(launch)


def _headline(exe, tmp_path, seed_mine, seed_other, count):
    mine, other = ML.gen(count, 10000, 0.05, seed_mine), ML.gen(count, 10000, 0.05, seed_other)
    q = FL.learned_q(FL.fit_model(other, 0))
    fit = FL.fit_model(mine, q)
    order = NL.library_order(mine)
    cut = [NL.max_cutoff(len(p), len(t), 15) for p, t in mine]

    def at(threshold, label):
        """threshold: None = none, an int, or "rhat" = the result the fit is made for"""
        launch = []
        for i in order:
            c1 = fit[i]["cut1"]
            p = c1 if threshold is None else min(c1, FL.rhat(q, cut[i]) if threshold == "rhat" else threshold)
            launch.append((i, c1, p, cut[i]))
        path = os.path.join(str(tmp_path), f"headline_{seed_mine}_{label}.bin")
        PL.write_launch(path, mine, launch)
        counts, rows, code, out = PL.walk(exe, path, 1, 1)
        assert code == 0 and counts["diffs"] == 0, out[-2000:]
        return counts, rows
    return q, fit, at


def test_headline_pairs_at_the_fitted_result(exe, tmp_path):
    """256 pairs of the headline's shape fitted from the other seed, thresholds at r^: no miss, fewer live slots"""
    for a, b in ((7101, 7102), (7102, 7101)):
        q, fit, at = _headline(exe, tmp_path, a, b, 256)
        base, _ = at(None, "none")
        pruned, rows = at("rhat", "rhat")
        print("seed", a, "q", q, "live slots per lane per chunk %.3f -> %.3f" % (base["live"] / base["lane_chunks"], pruned["live"] / pruned["lane_chunks"]),
              "block-columns %.4f" % (sum(r[1] for r in rows) / sum(r["adv1"] for r in fit)))
        assert not any(r["miss"] for r in fit)
        assert pruned["rejected"] == 0 and pruned["lost"] == 0 and [r[0] for r in rows] == [fit[i]["score"] for i in NL.library_order(ML.gen(256, 10000, 0.05, a))]
        assert pruned["live"] < base["live"] and pruned["lane_chunks"] == base["lane_chunks"]


def test_headline_table(exe, tmp_path):
    """the table of the change's note: 512 pairs of bench.py's generator and seed, fitted from another seed"""
    q, fit, at = _headline(exe, tmp_path, 0x51CED, 7102, 512)
    dist = [r["score"] for r in fit]
    print("q", q, "distances", min(dist), "..", max(dist), "cut1", min(r["cut1"] for r in fit), "..", max(r["cut1"] for r in fit))
    live, adv = {}, {}
    for thr in (None, 520, 510, 501, "rhat"):
        c, rows = at(thr, str(thr))
        ch = c["chunks"]
        live[thr], adv[thr] = c["live"], sum(r[1] for r in rows)
        print("threshold", thr, "live slots per lane per chunk %.2f" % (c["live"] / c["lane_chunks"]),
              "passes per chunk 4 / 2 / 1: %.2f / %.2f / %.2f" % (c["passes4"] / ch, c["passes2"] / ch, c["passes1"] / ch),
              "accepted", c["accepted"], "rejected", c["rejected"])
    print("block-columns of the first pass at r^ against none: %d / %d = %.4f" % (adv["rhat"], adv[None], adv["rhat"] / adv[None]))
    assert live["rhat"] < live[501] <= live[510] <= live[520] <= live[None]


def test_walk_under_sanitizers(tmp_path):
    """the program is host code with its own main: built once with ASan + UBSan and run on the smallest cases"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    san = PL.build_walk(str(tmp_path), sanitize=True)
    for name in ("last_row", "ragged_symbols"):
        pairs, _, _, launches = ML.case(name)
        full = [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in pairs]
        path = os.path.join(str(tmp_path), name + ".bin")
        PL.write_launch(path, pairs, [(i, c1, max(1, c1 * (30 + 20 * (k % 3)) // 100), full[i]) for k, (i, c1) in enumerate(launches[0])])
        counts, rows, code, out = PL.walk(san, path, 1, 1)
        assert code == 0 and counts["diffs"] == 0, out[-4000:]
        assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
