"""Band state in LDS (QE_SCORE_LDS), the part that needs no GPU: the ring of scores[] and the slot budget of
qe_types.h (score_lds_*).  tests/native/score_ring_cpu.cpp walks the kernel's chunk loop twice per group of 64 tasks, through
plain arrays and through a slice laid out as k_banded<false, true> lays it out, and checks that every eligible task's score
and block-advances agree, that no access leaves its chunk's window (shorter than the ring by two), that every row read is the
row last written at its ring index, and that the read-out finds row nw - 1.  `pytest -s` prints the counts."""
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
CAP, RING = 13, 16


def build_walk(out_dir, sanitize=False):
    return native_build.build_walk("score_ring_cpu", out_dir, sanitize)


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
    return build_walk(str(tmp_path_factory.mktemp("score_ring")))


def _cases():
    """(pattern, text, cutoff): narrow_lib's random shapes, ragged and floor-cutoff sets"""
    out = [(p, t, c) for p, t, c in NL.random_shapes(seed=3, rounds=150)]
    out += [(p, t, NL.max_cutoff(len(p), len(t), 15)) for _, p, t in NL.ragged_pairs()]
    out += [(p, t, c) for _, p, t, c in NL.floor_cutoffs()]
    return out


def _launch_of(pairs, cutoffs, pruned):
    """every task at its fitted cutoffs for the four ratios and at its own cutoff (a task that keeps C), in the order of the
    pairs; pruned: the threshold of the same ratio where narrow_prune gives one"""
    launch = []
    for i, ((p, t), c) in enumerate(zip(pairs, cutoffs)):
        m, n = len(p), len(t)
        for q in QS:
            c1 = FL.fit_lane(m, n, c, q, FL.fit_slots(m, n, c, FL.rhat(q, c)))
            launch.append((i, c1, PL.prune_of(m, n, c, c1, q) if pruned else c1, c))
        launch.append((i, c, c, c))
    return launch


def _check(counts, rows, code, out, launch, pairs):
    assert code == 0, out[-3000:]
    assert counts["diffs"] == 0 and counts["rule_diffs"] == 0 and counts["bad_slot"] == 0 and counts["bad_row"] == 0 and counts["stale"] == 0
    assert len(rows) == len(launch) and counts["eligible"] + counts["rejected"] == len(launch)
    for (i, c1, _, _), (_, _, eligible) in zip(launch, rows):
        assert eligible == (NL.slots(len(pairs[i][0]), len(pairs[i][1]), c1) <= CAP)


def test_the_budget_is_one_definition(tmp_path):
    L = native_build.host_lib(str(tmp_path), "budget",
                              'extern "C" int b_cap() { return qe::score_lds_cap(); }\nextern "C" int b_ring() { return qe::score_lds_ring(); }\n'
                              'extern "C" int b_fits(int s) { return qe::score_lds_fits(s) ? 1 : 0; }\nextern "C" int b_row(int r) { return qe::score_lds_row(r); }\n'
                              'extern "C" int b_bytes(int s) { return qe::score_lds_bytes(s); }\n')
    assert (L.b_cap(), L.b_ring()) == (CAP, RING) and RING & (RING - 1) == 0
    assert CAP + 1 <= RING - 2                                   # a chunk's window of slots + 1 rows is shorter than the ring by two
    assert [s for s in range(0, 40) if L.b_fits(s)] == list(range(1, CAP + 1))
    assert all(L.b_row(r) == r % RING for r in range(0, 5000, 7))
    assert L.b_bytes(CAP) == 14 * 16 * 64 + RING * 4 * 64 == 18432
    assert 2 * 4 * L.b_bytes(CAP) <= 160 * 1024 < 3 * 54 * 1024    # two workgroups of four waves per CU, as the 54 KB pin has it


@pytest.mark.parametrize("pruned", [False, True])
def test_ring_walk_equals_plain_arrays_on_random_shapes(exe, tmp_path, pruned):
    cases = _cases()
    pairs = [(p, t) for p, t, _ in cases]
    launch = _launch_of(pairs, [c for _, _, c in cases], pruned)
    path = os.path.join(str(tmp_path), "shapes.bin")
    eligible = rejected = 0
    for k in range(0, len(launch), 64 * 24):
        part = launch[k:k + 64 * 24]
        PL.write_launch(path, pairs, part)
        counts, rows, code, out = walk(exe, path, 1, 1)
        _check(counts, rows, code, out, part, pairs)
        eligible += counts["eligible"]; rejected += counts["rejected"]
    print("random shapes, ragged, floor cutoffs; pruned", pruned, "tasks", len(launch), "eligible", eligible, "rejected by the budget", rejected)
    assert eligible > 1000 and rejected > 100


@pytest.mark.parametrize("lane_rel", [1, 0])
@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("name", MASKED_CASES)
def test_ring_walk_on_the_masked_cases(exe, tmp_path, name, pruned, lane_rel):
    pairs, _, _, _ = ML.case(name)
    order = NL.library_order(pairs)
    ordered = [pairs[i] for i in order]
    launch = _launch_of(ordered, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in ordered], pruned)
    path = os.path.join(str(tmp_path), f"{name}.bin")
    PL.write_launch(path, ordered, launch)
    counts, rows, code, out = walk(exe, path, lane_rel, 1)
    print(name, "pruned", pruned, "lane_rel", lane_rel, out.strip().splitlines()[0])
    _check(counts, rows, code, out, launch, ordered)
    assert counts["eligible"] > 0
    if name == "indels":
        assert counts["rejected"] > 0                            # 10 kb at C = 1 500: 25 slots


def test_walk_under_sanitizers(tmp_path):
    """the program is host code with its own main: built once with ASan + UBSan and run on the two smallest cases"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    san = build_walk(str(tmp_path), sanitize=True)
    for name in ("last_row", "ragged_symbols"):
        pairs, _, _, _ = ML.case(name)
        launch = _launch_of(pairs, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in pairs], True)
        path = os.path.join(str(tmp_path), name + ".bin")
        PL.write_launch(path, pairs, launch)
        counts, rows, code, out = walk(san, path, 1, 1)
        _check(counts, rows, code, out, launch, pairs)
        assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
