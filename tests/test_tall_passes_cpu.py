"""Tall passes of k_banded<false, true> (QE_SCORE_TALL), the part that needs no GPU.  tests/native/tall_plan_cpu.cpp
walks every group of 64 tasks twice through a slice laid out as the LDS form lays it out (scores[] through the ring of
score_lds_row): with the 4 / 2 / 1 plan alone, and with the kernel's tall plan in front of it (qe_types.h: tall_height,
pass_plan).  Per task the two walks must agree on the score, first / last / pos_v and the block advances; no access of either
may leave the window first + pos_v .. last + pos_v + 1 of its chunk or find a stale row.  Over all inputs the plan must take a
pass of every height 5 .. 10 and split a band of 11-13 slots.  `pytest -s` prints the counts and, for 256 pairs of the
headline, the passes per chunk by height."""
import os
import re
import shutil
import subprocess

import pytest

import masked_lib as ML
import narrow_fit_lib as FL
import narrow_lib as NL
import narrow_prune_lib as PL
import native_build

QS = (90, 200, 340, 520)            # the ratios of tests/test_narrow_fit_cpu.py
MASKED_CASES = ("interleaved", "indels", "ragged_symbols", "last_row", "fit_interleaved")
HEIGHTS = tuple(range(5, 11))       # qe_types.h: QE_TALL_MIN .. QE_TALL_MAX
CAP = 13


def build_walk(out_dir, sanitize=False):
    return native_build.build_walk("tall_plan_cpu", out_dir, sanitize)


def walk(exe, path, lane_rel=1, masked=1):
    """-> the program's counts, its lines per pair as [(score, adv, eligible)], its exit code and the rest of its output"""
    r = subprocess.run([exe, path, str(lane_rel), str(masked)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    rows, rest = [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "pair":
            rows.append((int(w[3]), int(w[5]), int(w[7])))
        else:
            rest.append(line)
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", rest[0])} if rest else {}
    return counts, rows, r.returncode, "\n".join(rest) + r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    return build_walk(str(tmp_path_factory.mktemp("tall_plan")))


@pytest.fixture(scope="module")
def taken():
    """the passes of every height, the splits and the dead lanes the plan took over the module's inputs, summed as the tests run"""
    return {}


def _add(taken, counts):
    for k in [f"tall{h}" for h in HEIGHTS] + ["splits", "whole", "fallbacks", "dead_lanes"]:
        taken[k] = taken.get(k, 0) + counts[k]


def _cases():
    """(pattern, text, cutoff): narrow_lib's random shapes, ragged, symbol and floor-cutoff sets"""
    out = [(p, t, c) for p, t, c in NL.random_shapes(seed=3, rounds=150)]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.ragged_pairs()]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.symbol_pairs()]
    out += [(p, t, c) for _, p, t, c in NL.floor_cutoffs()]
    return out


def _launch_of(pairs, cutoffs, pruned):
    """every task at its fitted cutoffs for the four ratios, in the order of the pairs; pruned: the threshold of the same
    ratio where narrow_prune gives one"""
    launch = []
    for i, ((p, t), c) in enumerate(zip(pairs, cutoffs)):
        m, n = len(p), len(t)
        for q in QS:
            c1 = FL.fit_lane(m, n, c, q, FL.fit_slots(m, n, c, FL.rhat(q, c)))
            launch.append((i, c1, PL.prune_of(m, n, c, c1, q) if pruned else c1, c))
    return launch


def _check(counts, rows, code, out, launch, pairs):
    assert code == 0, out[-3000:]
    assert counts["diffs"] == 0 and counts["rule_diffs"] == 0 and counts["bad_slot"] == 0 and counts["bad_row"] == 0 and counts["stale"] == 0
    assert len(rows) == len(launch) and counts["eligible"] + counts["rejected"] == len(launch)
    for (i, c1, _, _), (_, _, eligible) in zip(launch, rows):
        assert eligible == (NL.slots(len(pairs[i][0]), len(pairs[i][1]), c1) <= CAP)
    # a chunk is walked by one tall pass alone, by a tall pass and the old plan (a split), or by the old plan
    assert counts["whole"] + counts["splits"] == sum(counts[f"tall{h}"] for h in HEIGHTS)


def test_the_height_rule(tmp_path):
    """qe_types.h: tall_height compiled for the host: the walk itself at 5 .. 10 slots, the largest height whose remainder is
    0, 1, 2 or at least 4 slots above that, nothing below 5"""
    L = native_build.host_lib(str(tmp_path), "height",
                              'extern "C" int t_height(int h) { return qe::tall_height(h); }\n'
                              'extern "C" int t_min() { return qe::QE_TALL_MIN; }\nextern "C" int t_max() { return qe::QE_TALL_MAX; }\n')
    assert (L.t_min(), L.t_max()) == (HEIGHTS[0], HEIGHTS[-1])
    assert [L.t_height(h) for h in range(-3, 5)] == [0] * 8
    assert [L.t_height(h) for h in HEIGHTS] == list(HEIGHTS)
    assert [L.t_height(h) for h in (11, 12, 13, 14, 15, 16, 40)] == [10, 10, 9, 10, 10, 10, 10]
    for h in range(5, 64):
        assert h - L.t_height(h) in (0, 1, 2) or h - L.t_height(h) >= 4


@pytest.mark.parametrize("pruned", [False, True])
def test_tall_walk_equals_the_old_plan_on_random_shapes(exe, tmp_path, taken, pruned):
    cases = _cases()
    pairs = [(p, t) for p, t, _ in cases]
    launch = _launch_of(pairs, [c for _, _, c in cases], pruned)
    path = os.path.join(str(tmp_path), "shapes.bin")
    total = {}
    for k in range(0, len(launch), 64 * 24):
        part = launch[k:k + 64 * 24]
        PL.write_launch(path, pairs, part)
        counts, rows, code, out = walk(exe, path, 1, 1)
        _check(counts, rows, code, out, part, pairs)
        _add(taken, counts)
        for key, v in counts.items():
            total[key] = total.get(key, 0) + v
    print("random shapes, ragged, symbols, floor cutoffs; pruned", pruned, "tasks", len(launch),
          {k: total[k] for k in ("eligible", "rejected", "chunks", "whole", "splits", "fallbacks", "dead_lanes") + tuple(f"tall{h}" for h in HEIGHTS)})
    assert total["eligible"] > 1000 and total["whole"] > 0 and total["fallbacks"] > 0


@pytest.mark.parametrize("lane_rel", [1, 0])
@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("name", MASKED_CASES)
def test_tall_walk_on_the_masked_cases(exe, tmp_path, taken, name, pruned, lane_rel):
    pairs, _, _, _ = ML.case(name)
    order = NL.library_order(pairs)
    ordered = [pairs[i] for i in order]
    launch = _launch_of(ordered, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in ordered], pruned)
    path = os.path.join(str(tmp_path), f"{name}.bin")
    PL.write_launch(path, ordered, launch)
    counts, rows, code, out = walk(exe, path, lane_rel, 1)
    print(name, "pruned", pruned, "lane_rel", lane_rel, out.strip().splitlines()[0])
    _check(counts, rows, code, out, launch, ordered)
    _add(taken, counts)
    assert counts["eligible"] > 0


def _tall_bands():
    """generated pairs for what the sets above do not reach: 70 pairs each of 4 .. 10 kb at 5 % fitted to themselves (bands of
    5 .. 10 slots) and the 10 kb ones at half their cutoff (13 slots: the split of a band taller than the tallest pass)"""
    out = []
    for length in (4000, 5000, 6000, 7000, 8000, 10000):
        pairs = ML.gen(70, length, 0.05, 8400 + length // 1000)
        k = FL.learned_q(FL.fit_model(pairs, 0))
        fit = FL.fit_model(pairs, k)
        cut = [NL.max_cutoff(len(p), len(t), 15) for p, t in pairs]
        order = NL.library_order(pairs)
        for kp in (0, k):
            out.append((f"{length}_fit_{kp}", pairs, [(i, fit[i]["cut1"], PL.prune_of(len(pairs[i][0]), len(pairs[i][1]), cut[i], fit[i]["cut1"], kp), cut[i]) for i in order]))
        if length == 10000:
            half = [NL.narrow_cutoff(len(p), len(t), c) for (p, t), c in zip(pairs, cut)]
            out.append(("10000_half", pairs, [(i, half[i], half[i], cut[i]) for i in order]))
    return out


def test_every_height_is_taken_and_a_taller_band_is_split(exe, tmp_path, taken):
    for name, pairs, launch in _tall_bands():
        path = os.path.join(str(tmp_path), f"{name}.bin")
        PL.write_launch(path, pairs, launch)
        counts, rows, code, out = walk(exe, path, 1, 1)
        print(name, out.strip().splitlines()[0])
        _check(counts, rows, code, out, launch, pairs)
        _add(taken, counts)
        if name == "10000_half":
            assert {NL.slots(len(pairs[i][0]), len(pairs[i][1]), c1) for i, c1, _, _ in launch} == {CAP}
            assert counts["splits"] > 0
    print("taken over the module's inputs so far:", taken)
    for h in HEIGHTS:
        assert taken[f"tall{h}"] > 0, (h, taken)
    assert taken["splits"] > 0 and taken["dead_lanes"] > 0 and taken["fallbacks"] > 0


def test_headline_histogram(exe, tmp_path):
    """256 pairs of bench.py's generator and seed, fitted from another seed and pruned at the fitted result (as
    tests/test_narrow_prune_cpu.py's table): the passes per chunk by height, old plan and tall plan"""
    mine, other = ML.gen(256, 10000, 0.05, 0x51CED), ML.gen(256, 10000, 0.05, 7102)
    q = FL.learned_q(FL.fit_model(other, 0))
    fit = FL.fit_model(mine, q)
    cut = [NL.max_cutoff(len(p), len(t), 15) for p, t in mine]
    launch = [(i, fit[i]["cut1"], min(fit[i]["cut1"], FL.rhat(q, cut[i])), cut[i]) for i in NL.library_order(mine)]
    path = os.path.join(str(tmp_path), "headline.bin")
    PL.write_launch(path, mine, launch)
    counts, rows, code, out = walk(exe, path, 1, 1)
    _check(counts, rows, code, out, launch, mine)
    ch = counts["chunks"]
    print("headline, 256 pairs, q", q, "chunks", ch, "live slots per lane and chunk %.2f" % (counts["live"] / counts["lane_chunks"]))
    print("old plan, passes per chunk 4 / 2 / 1: %.3f / %.3f / %.3f" % (counts["old4"] / ch, counts["old2"] / ch, counts["old1"] / ch))
    print("tall plan, passes per chunk " + " ".join("%d: %.3f" % (h, counts[f"tall{h}"] / ch) for h in HEIGHTS) +
          "; beside them 4 / 2 / 1: %.3f / %.3f / %.3f" % (counts["passes4"] / ch, counts["passes2"] / ch, counts["passes1"] / ch) +
          "; chunks left to the old plan %.3f" % (1 - (counts["whole"] + counts["splits"]) / ch))
    total_old = counts["old4"] + counts["old2"] + counts["old1"]
    total_new = counts["passes4"] + counts["passes2"] + counts["passes1"] + counts["whole"] + counts["splits"]
    assert total_new < total_old and counts["whole"] > ch // 2


def test_walk_under_sanitizers(tmp_path):
    """the program is host code with its own main: built once with ASan + UBSan and run on the two smallest cases and on a
    wave of bands taller than the old plan's passes"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    san = build_walk(str(tmp_path), sanitize=True)
    runs = []
    for name in ("last_row", "ragged_symbols"):
        pairs, _, _, _ = ML.case(name)
        runs.append((name, pairs, _launch_of(pairs, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in pairs], True)))
    pairs = ML.gen(6, 10000, 0.05, 8410)
    cut = [NL.max_cutoff(len(p), len(t), 15) for p, t in pairs]
    runs.append(("tall", pairs, [(i, c1, c1, cut[i]) for i in range(6) for c1 in (330, 400, 520, 750)]))
    for name, pairs, launch in runs:
        path = os.path.join(str(tmp_path), name + ".bin")
        PL.write_launch(path, pairs, launch)
        counts, rows, code, out = walk(san, path, 1, 1)
        _check(counts, rows, code, out, launch, pairs)
        assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
        if name == "tall":
            assert counts["whole"] > 0 and counts["splits"] > 0
