#!/usr/bin/env python3
"""All-occurrences runs (quicked_batch_run_search_all): what the feature costs next to the best search, and next to the loop a
caller needs without it to get a second occurrence.

    python tools/search_hits_bench.py [--rounds 7] [--cap 4] --out profiles/search_hits.json

The data are search_bench.py's leg a: 1 000 000 pairs, a 150-base pattern in a 400-base text, 4 %, bound 12, INFIX.  Three
ways, alternating round by round in one process, synchronous runs (queue depth 1), one warm-up round dropped, min / median /
max over the rounds; every way is timed until its answers are in numpy arrays:
    best   quicked_batch_run_search + scores + locations
    all    quicked_batch_run_search_all with the cap + hits
    loop   best, then on the host every text cut behind its located stretch (offset and length arithmetic: the pools are not
           copied), the cut pairs reloaded into a second batch object, and best again on that one
Per block step (64 rows x 1 column): quicked_batch_kernel_times()[0] over quicked_batch_counters()[0] of one run of `best`
and of `all` -- the all-occurrences forward pass cannot lower its bound or stop at an exact occurrence, so it computes more of
them.  The verdict compares the medians of `all` and `loop` with the larger of their two spreads (max - min).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cap", type=int, default=4)
    ap.add_argument("--count", type=int, default=0, help="override the number of pairs (smoke runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    import search_bench as SB
    from quicked_amd import capi, datagen
    leg = dict(SB.LEGS["a"])
    if args.count:
        leg["count"] = args.count
    os.environ.pop("QE_SEARCH_FORM", None)
    base = datagen.generate(leg["count"], leg["m"], leg["error"], seed=leg["seed"])
    batch = SB.embed(base, leg["n"], leg["seed"] + 1000, datagen)
    bound, mode, n = leg["bound"], capi.SEARCH_INFIX, leg["count"]
    rb = capi.ResidentBatch(batch)
    rb2 = capi.ResidentBatch(batch)               # the loop's second batch object: reloaded every round

    def best(b):
        if b.run_search(mode, bound, only_score=True, sync=True) < 0:
            raise RuntimeError("quicked_batch_run_search failed")
        sc, _ = b.scores()
        ts, te = b.locations()
        return sc, ts, te

    def every():
        if rb.run_search_all(mode, bound, max_hits=args.cap, sync=True) < 0:
            raise RuntimeError("quicked_batch_run_search_all failed")
        return rb.hits()

    def loop():
        sc, ts, te = best(rb)
        end = np.where(te > 0, te, batch.text_len).astype(np.int64)          # nothing found: nothing left to search
        cut = datagen.PairBatch(batch.pattern_pool, batch.pattern_off, batch.pattern_len, batch.text_pool, batch.text_off + end,
                                (batch.text_len - end).astype(np.int32))
        if rb2.reload(cut) < 0:
            raise RuntimeError("quicked_batch_reload failed")
        sc2, ts2, te2 = best(rb2)
        return sc, ts, te, sc2, ts2 + end.astype(np.int32), te2 + end.astype(np.int32)

    # the answers agree where they must: the smallest stored occurrence of an uncapped-enough run is the best search's
    per_step = {}
    rb.kernel_times()
    sc, ts, te = best(rb)
    ms, launches = rb.kernel_times()
    steps = int(rb.counters()[0])
    per_step["best"] = dict(kernel_ms=round(float(ms[0]), 4), launches=int(launches[0]), block_steps=steps,
                            ps_per_block_step=round(float(ms[0]) * 1e9 / max(steps, 1), 3))
    found, off, hits = every()
    ms, launches = rb.kernel_times()
    steps = int(rb.counters()[0])
    per_step["all"] = dict(kernel_ms=round(float(ms[0]), 4), launches=int(launches[0]), block_steps=steps,
                           ps_per_block_step=round(float(ms[0]) * 1e9 / max(steps, 1), 3))
    sc_all, _ = rb.scores()
    assert (sc_all == sc).all(), "the smallest score among the occurrences is not the best search's"
    first = off[:-1][found > 0]
    assert (hits["text_end"][first] <= te[found > 0]).all()

    ways = {"best": lambda: best(rb), "all": every, "loop": loop}
    times = {k: [] for k in ways}
    for rnd in range(args.rounds + 1):
        for name, fn in ways.items():
            rb.sync()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rnd > 0:                              # round 0 warms pools, streams and clocks up
                times[name].append(dt * 1e3)
    out = dict(pairs=n, pattern=leg["m"], text=leg["n"], error=leg["error"], bound=bound, mode="infix", cap=args.cap, rounds=args.rounds,
               unit="ms per synchronous run, answers in numpy arrays", within=int((sc >= 0).sum()),
               occurrences_found=int(found.sum()), occurrences_stored=int(off[-1]), pairs_with_more_than_one=int((found > 1).sum()),
               ways={}, kernel=per_step)
    for k, v in times.items():
        out["ways"][k] = dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), samples=[round(x, 4) for x in v])
    a, lp = out["ways"]["all"], out["ways"]["loop"]
    spread = max(a["max"] - a["min"], lp["max"] - lp["min"])
    out["block_step_ratio_all_over_best"] = round(per_step["all"]["block_steps"] / max(1, per_step["best"]["block_steps"]), 3)
    out["larger_spread_ms"] = round(spread, 4)
    out["all_beats_loop_by_more_than_the_spread"] = bool(lp["median"] - a["median"] > spread)
    rb.close()
    rb2.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
