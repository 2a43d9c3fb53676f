#!/usr/bin/env python3
"""Search runs (quicked_batch_run_search): the two kernel forms against each other and against edlib on the host's CPUs.

    python tools/search_bench.py --leg a [--rounds 7] [--steps 4] --out profiles/search_a.json

Legs (device-resident batch, queued runs timed as bench.py's headline does: `steps` runs with sync=False, one sync):
    a   1 000 000 pairs, pattern 150 in text 400, 4 %, bound 12, INFIX
    b   100 000 pairs, pattern 10 kb in text 12 kb, 5 %, bound 1 000, INFIX   (the workspace form only: 157 blocks)
    c   leg a's data as PREFIX
    m64 / m128 / m256   leg a's shape with patterns of 1, 2 and 4 blocks: where does the register form pay?
The forms (QE_SEARCH_FORM = 0 workspace, 1 registers) alternate round by round in one process; one warm-up round is
dropped; min / median / max over the rounds are reported, and the forms must give the same answers on the timed input.
Nothing in a tree without the mode computes these answers, so the yardsticks are outside it:
  * edlib HW / SHW with EDLIB_TASK_LOC and the same bound (oracle/_ref/libedlib_ref.so, where it is built; else the column
    is left out) on 16 threads, one per core, over the same pairs -- or over the first --edlib-pairs of them, as a rate; the
    loop over the pairs is compiled code (tools/search_edlib.cpp);
  * per block step (64 rows x 1 column): the search kernels' time from quicked_batch_kernel_times()[0] over
    quicked_batch_counters()[0], next to the same ratio of a BANDED only_score run (k_banded<false>) on pairs of the pattern's
    length (--banded-ref).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = {"a": dict(count=1_000_000, m=150, n=400, error=0.04, bound=12, mode="infix", seed=21),
        "b": dict(count=100_000, m=10_000, n=12_000, error=0.05, bound=1000, mode="infix", seed=22),
        "c": dict(count=1_000_000, m=150, n=400, error=0.04, bound=12, mode="prefix", seed=21),
        "m64": dict(count=1_000_000, m=64, n=400, error=0.04, bound=6, mode="infix", seed=23),
        "m128": dict(count=1_000_000, m=128, n=400, error=0.04, bound=10, mode="infix", seed=24),
        "m256": dict(count=1_000_000, m=256, n=400, error=0.04, bound=20, mode="infix", seed=25)}


def embed(batch, n, seed, datagen):
    """every text of `batch` (a mutated copy of its pattern) inside a random text of exactly n bases, at a random place"""
    rng = np.random.default_rng(seed)
    count = len(batch)
    tl = batch.text_len.astype(np.int64)
    assert int(tl.max()) <= n, "a mutated pattern is longer than the text"
    left = (rng.random(count) * (n - tl + 1)).astype(np.int64)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, count * n, dtype=np.uint8)]
    new_off = np.arange(count, dtype=np.int64) * n
    step = max(1, (1 << 26) // max(1, int(tl.max())))          # a slice of pairs at a time: the index array stays small
    for lo in range(0, count, step):
        hi = min(count, lo + step)
        first, end = int(batch.text_off[lo]), int(batch.text_off[hi - 1] + tl[hi - 1])
        shift = new_off[lo:hi] + left[lo:hi] - batch.text_off[lo:hi]
        pool[np.repeat(shift, tl[lo:hi]) + np.arange(first, end, dtype=np.int64)] = batch.text_pool[first:end]
    return datagen.PairBatch(batch.pattern_pool, batch.pattern_off, batch.pattern_len, pool, new_off, np.full(count, n, dtype=np.int32))


def edlib_rate(batch, mode, bound, pairs, threads=16):
    """-> (pairs per second, [d, start, end] of the pairs done) or None where the library is absent; the loop over the
    pairs is tools/search_edlib.cpp's, built into tools/bin/ on first use"""
    import ctypes as C
    import subprocess
    import search_lib as S
    if not S.have_edlib():
        return None
    so = os.path.join(ROOT, "tools", "bin", "libsearch_edlib.so")
    src = os.path.join(ROOT, "tools", "search_edlib.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", src, "-ldl", "-o", so], check=True)
    lib = C.CDLL(so)
    lib.search_edlib_run.restype = C.c_double
    lib.search_edlib_run.argtypes = [C.c_char_p, C.c_int64] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
    pairs = min(pairs, len(batch))
    out = np.full((pairs, 3), -1, dtype=np.int32)
    sec = lib.search_edlib_run(S.EDLIB_SO.encode(), pairs, batch.pattern_pool.ctypes.data, batch.pattern_off.ctypes.data,
                               batch.pattern_len.ctypes.data, batch.text_pool.ctypes.data, batch.text_off.ctypes.data,
                               batch.text_len.ctypes.data, S.EDLIB_MODE[mode], int(min(bound, 2**31 - 1)), threads, out.ctypes.data)
    return (pairs / sec, out) if sec > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--count", type=int, default=0, help="override the leg's number of pairs (smoke runs)")
    ap.add_argument("--edlib-pairs", type=int, default=1_000_000, help="pairs edlib is timed on (0: no edlib column)")
    ap.add_argument("--banded-ref", action="store_true", help="time a BANDED only_score run on pairs of the pattern's length too")
    ap.add_argument("--out")
    args = ap.parse_args()
    leg = dict(LEGS[args.leg])
    if args.count:
        leg["count"] = args.count
    os.environ.pop("QE_SEARCH_FORM", None)
    os.environ.pop("QUICKED_HIP_LIB", None)

    from quicked_amd import capi, datagen
    mode = capi.SEARCH_INFIX if leg["mode"] == "infix" else capi.SEARCH_PREFIX
    base = datagen.generate(leg["count"], leg["m"], leg["error"], seed=leg["seed"])
    batch = embed(base, leg["n"], leg["seed"] + 1000, datagen)
    bound = leg["bound"]
    rb = capi.ResidentBatch(batch)
    reg_applies = leg["m"] <= 256
    forms = {"workspace": "0"}
    if reg_applies:
        forms["registers"] = "1"

    def prepare(switch):
        os.environ["QE_SEARCH_FORM"] = switch
        capi.reload_env()

    # the same answers first; per-block-step cost from the kernel events and the step counter of one sync run
    ans, per_step = {}, {}
    for name, switch in forms.items():
        prepare(switch)
        rb.kernel_times()
        assert rb.run_search(mode, bound, only_score=True, sync=True) >= 0
        ms, launches = rb.kernel_times()
        steps = int(rb.counters()[0])
        sc = rb.scores()[0]
        ts, te = rb.locations()
        ans[name] = np.stack([sc, ts, te], axis=1)
        per_step[name] = dict(kernel_ms=round(float(ms[0]), 4), launches=int(launches[0]), block_steps=steps,
                              ps_per_block_step=round(float(ms[0]) * 1e9 / max(steps, 1), 3))
    ref = ans["workspace"]
    for name, a in ans.items():
        assert (a == ref).all(), f"{name} disagrees with workspace on {int((a != ref).any(axis=1).sum())} pairs"
    within = int((ref[:, 0] >= 0).sum())

    times = {k: [] for k in forms}
    for rnd in range(args.rounds + 1):
        for name, switch in forms.items():
            prepare(switch)
            rb.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if rb.run_search(mode, bound, only_score=True, sync=False) < 0:
                    raise RuntimeError("quicked_batch_run_search failed")
            rb.sync()
            dt = (time.perf_counter() - t0) / args.steps
            if rnd > 0:                              # round 0 warms pools, streams and clocks up
                times[name].append(dt * 1e3)
    os.environ.pop("QE_SEARCH_FORM", None)
    capi.reload_env()

    out = dict(leg=args.leg, pairs=leg["count"], pattern=leg["m"], text=leg["n"], error=leg["error"], bound=bound, mode=leg["mode"],
               within=within, rounds=args.rounds, steps_per_round=args.steps, unit="ms per queued run", forms={}, kernel=per_step)
    for k, v in times.items():
        out["forms"][k] = dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4),
                               mpairs_per_s=round(leg["count"] / statistics.median(v) / 1e3, 3), samples=[round(x, 4) for x in v])
    if args.banded_ref:
        gb = capi.ResidentBatch(base)
        gb.kernel_times()
        assert gb.run(capi.make_params(algo=capi.BANDED, only_score=True), sync=True) >= 0
        ms, launches = gb.kernel_times()
        steps = int(gb.counters()[0])
        out["banded_ref"] = dict(kernel_ms=round(float(ms[0]), 4), launches=int(launches[0]), block_steps=steps,
                                 ps_per_block_step=round(float(ms[0]) * 1e9 / max(steps, 1), 3))
        gb.close()
    if args.edlib_pairs:
        import search_lib as S
        r = edlib_rate(batch, S.INFIX if leg["mode"] == "infix" else S.PREFIX, bound, args.edlib_pairs)
        if r is not None:
            rate, got = r
            k = len(got)
            # edlib's d == m cases (end location -1) are outside the comparison, as in the tests
            cmp = (got[:, 0] != leg["m"]) | (ref[:k, 0] != leg["m"])
            assert (got[cmp] == ref[:k][cmp]).all(), "edlib disagrees with the library on the timed pairs"
            out["edlib"] = dict(threads=16, pairs=k, mpairs_per_s=round(rate / 1e6, 4))
    rb.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
