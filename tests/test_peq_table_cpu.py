"""Eq from a table (QE_SCORE_PEQ), the part that needs no GPU.  tests/native/peq_table_cpu.cpp checks the layout
functions of qe_types.h (peq_*) and walks every group of 64 tasks twice with the tall plan and the state by absolute block
row, as the table form keeps it: through tests/native/banded_walk.h as it is, and with every tall pass reading Eq from a
wave's slice built as the kernel builds it.  Per task the two walks must agree on the score, first / last / pos_v and the
block advances; no access of the table may leave the slice, read a word its own pass did not write, or meet a fifth symbol,
and every live entry must equal the compiled pattern's Eq word.  The inputs are those of tests/test_tall_passes_cpu.py; over
them a pass of every height 5 .. 10 must have read the table."""
import os
import re
import shutil
import subprocess

import pytest

import masked_lib as ML
import narrow_lib as NL
import narrow_prune_lib as PL
import native_build
import test_tall_passes_cpu as TP

HEIGHTS = TP.HEIGHTS


def walk(exe, path, lane_rel=1, masked=1):
    r = subprocess.run([exe, path, str(lane_rel), str(masked)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    rows = [line for line in r.stdout.splitlines() if line.startswith("pair ")]
    rest = [line for line in r.stdout.splitlines() if not line.startswith("pair ")]
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", rest[0])} if rest else {}
    return counts, len(rows), r.returncode, "\n".join(rest) + r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    return native_build.build_walk("peq_table_cpu", str(tmp_path_factory.mktemp("peq_table")))


@pytest.fixture(scope="module")
def taken():
    """the tall passes by height that read the table over the module's inputs, summed as the tests run"""
    return {}


def _check(counts, nrows, code, out, launch, taken):
    assert code == 0, out[-3000:]
    for key in ("diffs", "rule_diffs", "bad_off", "unwritten", "bad_sym", "mismatch", "tall_diff"):
        assert counts[key] == 0, (key, out[-2000:])
    assert nrows == len(launch) == counts["pairs"]
    tall = sum(counts[f"tall{h}"] for h in HEIGHTS)
    assert (counts["reads"] > 0) == (tall > 0) and counts["writes"] * 16 == counts["reads"]      # per lane and pass 4 K words written, 64 K read
    for key in [f"tall{h}" for h in HEIGHTS] + ["dead_lanes"]:
        taken[key] = taken.get(key, 0) + counts[key]


def test_the_layout(exe):
    """peq_entry against the plane formula for all (a, b, sym) bit cases, offsets apart and inside the slice, two workgroups of
    four slices in a CU's LDS, lane l on bank 2 l mod 64 whatever sym and slot"""
    r = subprocess.run([exe, "layout"], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    c = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", r.stdout)}
    assert c["bad"] == 0 and c["cap"] == HEIGHTS[-1] == 10
    assert c["sym_stride"] == 10 * 512 and c["sym_stride"] % 256 == 0 and c["bytes"] == 20 * 1024 and 2 * c["workgroup"] <= 160 * 1024


@pytest.mark.parametrize("pruned", [False, True])
def test_table_walk_equals_the_plane_walk_on_random_shapes(exe, tmp_path, taken, pruned):
    cases = TP._cases()
    pairs = [(p, t) for p, t, _ in cases]
    launch = TP._launch_of(pairs, [c for _, _, c in cases], pruned)
    path = os.path.join(str(tmp_path), "shapes.bin")
    tall = 0
    for k in range(0, len(launch), 64 * 24):
        part = launch[k:k + 64 * 24]
        PL.write_launch(path, pairs, part)
        counts, nrows, code, out = walk(exe, path, 1, 1)
        _check(counts, nrows, code, out, part, taken)
        tall += sum(counts[f"tall{h}"] for h in HEIGHTS)
    print("random shapes, ragged, symbols, floor cutoffs; pruned", pruned, "tasks", len(launch), "tall passes through the table", tall)
    assert tall > 0


@pytest.mark.parametrize("lane_rel", [1, 0])
@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("name", TP.MASKED_CASES)
def test_table_walk_on_the_masked_cases(exe, tmp_path, taken, name, pruned, lane_rel):
    pairs, _, _, _ = ML.case(name)
    ordered = [pairs[i] for i in NL.library_order(pairs)]
    launch = TP._launch_of(ordered, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in ordered], pruned)
    path = os.path.join(str(tmp_path), f"{name}.bin")
    PL.write_launch(path, ordered, launch)
    counts, nrows, code, out = walk(exe, path, lane_rel, 1)
    print(name, "pruned", pruned, "lane_rel", lane_rel, out.strip().splitlines()[0])
    _check(counts, nrows, code, out, launch, taken)


def test_every_height_reads_the_table(exe, tmp_path, taken):
    for name, pairs, launch in TP._tall_bands():
        path = os.path.join(str(tmp_path), f"{name}.bin")
        PL.write_launch(path, pairs, launch)
        counts, nrows, code, out = walk(exe, path, 1, 1)
        print(name, out.strip().splitlines()[0])
        _check(counts, nrows, code, out, launch, taken)
    print("taken over the module's inputs so far:", taken)
    for h in HEIGHTS:
        assert taken[f"tall{h}"] > 0, (h, taken)
    assert taken["dead_lanes"] > 0            # dead suffixes read rows of the table too


def test_walk_under_sanitizers(tmp_path):
    """the program is host code with its own main: built once more with ASan + UBSan and run stand-alone on the layout check,
    the two smallest masked cases and a wave of tall bands"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    san = native_build.build_walk("peq_table_cpu", str(tmp_path), sanitize=True)
    r = subprocess.run([san, "layout"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    runs = []
    for name in ("last_row", "ragged_symbols"):
        pairs, _, _, _ = ML.case(name)
        runs.append((name, pairs, TP._launch_of(pairs, [NL.max_cutoff(len(p), len(t), ML.BW) for p, t in pairs], True)))
    pairs = ML.gen(6, 10000, 0.05, 8410)
    cut = [NL.max_cutoff(len(p), len(t), 15) for p, t in pairs]
    runs.append(("tall", pairs, [(i, c1, c1, cut[i]) for i in range(6) for c1 in (330, 400, 520, 750)]))
    seen = {}
    for name, pairs, launch in runs:
        path = os.path.join(str(tmp_path), name + ".bin")
        PL.write_launch(path, pairs, launch)
        counts, nrows, code, out = walk(san, path, 1, 1)
        _check(counts, nrows, code, out, launch, seen)
        assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
        if name == "tall":
            assert sum(counts[f"tall{h}"] for h in HEIGHTS) > 0
