"""Masked multi-slot passes of k_banded<false> (QE_SCORE_MASKED): the cases the CPU test and the GPU test
share, and the stand-alone CPU walk (tests/native/pass_plan_cpu.cpp) that runs the kernel's pass plan over them with the
oracle's block step.  Test infrastructure only."""
import functools
import os
import re
import struct
import subprocess

import narrow_fit_lib as FL
import narrow_lib as NL
import native_build
from quicked_amd import datagen

BW = 15


def gen(count, length, error, seed, **kw):
    return list(datagen.generate(count=count, length=length, error=error, seed=seed, **kw).pairs())


def _interleaved():
    """3 kb reads at 1 / 4 / 8 / 12 % in turn (one length: the library keeps the order), so every wave holds bands whose
    heights differ by several slots"""
    sets = [gen(48, 3000, e, 6100 + i) for i, e in enumerate((0.01, 0.04, 0.08, 0.12))]
    return [s[i] for i in range(48) for s in sets]


def _ragged_symbols():
    """narrow_lib's ragged pairs (partial last chunks, both signs of m - n) and its N / lower-case / IUPAC pairs, with pairs
    of m mod 64 = 0, 1 and 63, among 64 plain 2 kb reads"""
    pairs = [(p, t) for _, p, t in NL.ragged_pairs()][::3] + [(p, t) for _, p, t in NL.symbol_pairs()]
    plain = gen(64, 2000, 0.04, 6200)
    for k, m in enumerate((1984, 1985, 1983, 1920, 1921, 1919)):
        plain[k] = (plain[k][0][:m], plain[k][1])
    out = []
    for i in range(max(len(pairs), len(plain))):
        out += pairs[i:i + 1] + plain[i:i + 1]
    return out


def _last_row():
    """1 kb reads whose patterns end 0 .. 3 block rows apart in turn: the text keeps its length, so the library keeps the
    order and every wave has lanes in their last block row next to lanes that are not"""
    return [(p[:len(p) - 64 * (i % 4)], t) for i, (p, t) in enumerate(gen(130, 1000, 0.06, 6300))]


def _fit_interleaved():
    """2 / 4 / 12 % reads of 3 kb in turn, fitted to the 2 % ones (tests/test_gpu_narrow_fit.py's interleaved case): bands of
    three slots next to bands at half the cutoff in every wave of the first launch, and a second launch over the misses"""
    sets = [gen(64, 3000, e, 5110 + i) for i, e in enumerate((0.02, 0.04, 0.12))]
    return [s[i] for i in range(64) for s in sets], FL.learned_q(FL.fit_model(sets[0], 0))


# name -> (pairs, the switches of the run besides those that force the one-lane kernel; QE_NARROW_FIT may be a function of the case)
CASES = {
    "interleaved": (_interleaved, {"QE_SCORE_NARROW": "0"}),
    "forced_fit": (lambda: gen(150, 3000, 0.02, 5101), {"QE_SCORE_NARROW": "1", "QE_NARROW_FIT": "137"}),
    "fit_interleaved": (lambda: _fit_interleaved()[0], {"QE_SCORE_NARROW": "1", "QE_NARROW_FIT": lambda: str(_fit_interleaved()[1])}),
    "ragged_symbols": (_ragged_symbols, {"QE_SCORE_NARROW": "0"}),
    "indels": (lambda: gen(70, 10000, 0.05, 6400, indels_num=2, indels_len=500), {"QE_SCORE_NARROW": "0"}),
    "indels_union_walk": (lambda: gen(70, 10000, 0.05, 6400, indels_num=2, indels_len=500), {"QE_SCORE_NARROW": "0", "QE_LANE_REL": "0"}),
    "last_row": (_last_row, {"QE_SCORE_NARROW": "0"}),
}
# the first launch of a fitted run of 3 kb reads walks three slots in every lane of every wave: nothing there to mask
UNIFORM_FIRST = ("forced_fit", "fit_interleaved")
ONE_LANE = {"QE_COOP_G": "1", "QE_WAVE": "0", "QE_SCORE_SYS": "0"}      # run_banded_score: neither cooperative, wave nor systolic form


@functools.lru_cache(maxsize=None)
def case(name):
    """-> pairs, switches, the oracle's model of the run (scores, counters[0], counters[7]), the launches the CPU walk
    checks as lists of (pair index in library order, cutoff) -- computed once, shared, never changed"""
    make, env = CASES[name]
    pairs = make()
    env = {k: (v() if callable(v) else v) for k, v in env.items()}
    order = NL.library_order(pairs)
    full = [NL.max_cutoff(len(p), len(t), BW) for p, t in pairs]
    if env["QE_SCORE_NARROW"] == "1":
        fit = FL.fit_model(pairs, int(env["QE_NARROW_FIT"]))
        expect = FL.totals(fit)
        # the second launch: the misses at their full cutoffs (here in library order; the device packs them as its waves arrive)
        again = [i for i in order if fit[i]["miss"]]
        launches = [[(i, fit[i]["cut1"]) for i in order]] + ([[(i, full[i]) for i in again]] if again else [])
    else:
        res = NL.two_pass_many(pairs, bandwidth=BW)
        expect = ([r["score"] for r in res], sum(r["adv"] for r in res), 0)
        launches = [[(i, full[i]) for i in order]]
    return pairs, dict(env), expect, launches


def headline_launches(count=256):
    """the headline's pairs (bench.py: 10 kb at 5 %, its seed) at the full cutoff, at half of it and at ten slots"""
    pairs = gen(count, 10000, 0.05, 0x51CED)
    order = NL.library_order(pairs)
    return pairs, {c: [(i, c) for i in order] for c in (1500, 750, 576)}


def write_launch(path, pairs, launch):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(launch)))
        for i, cutoff in launch:
            p, t = pairs[i]
            f.write(struct.pack("<iii", len(p), len(t), cutoff) + p + t)


def build_walk(out_dir, sanitize=False):
    return native_build.build_walk("pass_plan_cpu", out_dir, sanitize)


def walk(exe, path, lane_rel=1, masked=1):
    """-> the program's counts (diffs, rule_diffs, chunks, passes4 / 2 / 1, partial_passes), its exit code and its output"""
    r = subprocess.run([exe, path, str(lane_rel), str(masked)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", r.stdout.splitlines()[0])} if r.stdout else {}
    return counts, r.returncode, r.stdout + r.stderr
