#!/usr/bin/env python3
"""BandEd score-only in two passes on data it must not hurt: a stream of queued runs over pairs whose distances lie above
half the cutoff (10 %: every task misses the first pass; 8 %: about half do), against the parent commit's library.

    python tools/narrow_stream.py --error 0.10 --parent <tree of the parent commit, built> [--rounds 7] [--steps 16] --out profiles/narrow_10pct.json

Device-resident batch, runs queued as bench.py's headline queues them (`steps` runs with sync=False, one sync).  Pools and
streams are warmed with the switch forced both ways (QE_SCORE_NARROW = 1 / 0 leave the policy's verdicts alone); then, with
the default switch:
    first run       one synchronous run on data the policy knows nothing about (it takes the first pass), next to a
                    synchronous single-pass run of this tree (QE_SCORE_NARROW=0) and of the parent
    steady state    rounds of `steps` queued runs, this tree and the parent alternating round by round (--only this / parent:
                    one library per process, for alternating processes); with the default 16 steps a round holds exactly
                    one probe once the policy has left the first pass (--steady-switch 0 / -2: none)
    --reseed K      real use instead of one replayed batch: K resident batches per error rate, every one of another seed,
                    rotated, every run queued and fetched one run behind (so the policy and the fit see every run's counts);
                    --schedule 0.05:12,0.06:8,0.05:8 shifts the error rate in the stream.  One library per process
                    (--lib <libquicked_hip.so of the parent> for the baseline).  Reports every run's ms (fetch to fetch),
                    block-columns and second-pass tasks, the steps after each shift included, and min / median / max per
                    segment without its first two runs (the pipeline's fill and the run after a shift are listed, not hidden)
min / median / max of the ms per run over the rounds; counters[0] (block-columns advanced) and counters[7] (tasks of the
second pass) of a synchronous run after the rounds show what the policy settled on.  Scores must equal the parent's.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), samples=[round(x, 4) for x in v])


def reseeded(args):
    if args.lib:
        os.environ["QUICKED_HIP_LIB"] = os.path.abspath(args.lib)
    if args.steady_switch is not None:
        os.environ["QE_SCORE_NARROW"] = args.steady_switch
    from quicked_amd import capi, datagen
    sched = [(float(e), int(n)) for e, n in (x.split(":") for x in (args.schedule or "%g:24" % args.error).split(","))]
    params = capi.make_params(algo=capi.BANDED, only_score=True, bandwidth=args.bandwidth)
    rbs, checks = {}, {}
    for e in sorted({e for e, _ in sched}):
        for i in range(args.reseed):
            seed = args.seed + 1000 * int(round(e * 1000)) + i
            rbs[(e, i)] = capi.ResidentBatch(datagen.generate(args.count, args.length, e, seed=seed))
    # warm-up with the switch forced both ways on every batch (pools, code objects; the policy learns nothing from forced runs) ...
    for v in ("1", "0"):
        os.environ["QE_SCORE_NARROW"] = v
        capi.reload_env()
        for key, rb in rbs.items():
            if rb.run(params, sync=False) < 0 or rb.fetch() < 0:
                raise RuntimeError("warm-up run failed")
            if v == "0":
                checks[key] = rb.scores()[0].copy()               # the single pass's scores
    if args.steady_switch is None:
        os.environ.pop("QE_SCORE_NARROW", None)
    else:
        os.environ["QE_SCORE_NARROW"] = args.steady_switch
    capi.reload_env()                                             # ... and the stream starts from unknown data
    runs, prev, k = [], None, 0
    host_ms = []

    def finish(item):
        key, rb, seg = item
        if rb.fetch() < 0:
            raise RuntimeError("quicked_batch_fetch failed")
        c = rb.counters()
        assert (rb.scores()[0] == checks[key]).all(), "scores differ from the single pass's"
        runs.append(dict(segment=seg, error=key[0], batch=key[1], t=time.perf_counter(), block_columns=int(c[0]), second_pass_tasks=int(c[7])))

    t_start = time.perf_counter()
    for seg, (e, n) in enumerate(sched):
        for _ in range(n):
            key = (e, k % args.reseed)
            k += 1
            th = time.perf_counter()
            if rbs[key].run(params, sync=False) < 0:
                raise RuntimeError("quicked_batch_run failed")
            host_ms.append((time.perf_counter() - th) * 1e3)
            if prev:
                finish(prev)
            prev = (key, rbs[key], seg)
    finish(prev)
    last = t_start
    for r in runs:
        r["ms"] = round((r["t"] - last) * 1e3, 4)
        last = r.pop("t")
    out = dict(mode="reseeded", lib=os.environ.get("QUICKED_HIP_LIB", "this tree"), pairs=args.count, length=args.length,
               batches_per_error=args.reseed, schedule=sched, bandwidth=args.bandwidth, unit="ms per run (fetch to fetch)",
               host_ms_per_queued_run=stats(host_ms), runs=runs, segments=[])
    for seg, (e, n) in enumerate(sched):
        mine = [r for r in runs if r["segment"] == seg]
        out["segments"].append(dict(error=e, runs=n, ms_without_first_two=stats([r["ms"] for r in mine[2:]]) if len(mine) > 2 else None,
                                    ms_first_two=[r["ms"] for r in mine[:2]], second_pass_tasks=[r["second_pass_tasks"] for r in mine],
                                    block_columns_last=mine[-1]["block_columns"]))
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    for rb in rbs.values():
        rb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=10_000)
    ap.add_argument("--error", type=float, default=0.10)
    ap.add_argument("--bandwidth", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0x51CED)
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no baseline)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--only", choices=["both", "this", "parent"], default="both",
                    help="time one library per process (two libraries in one process share the runtime's hardware queues: "
                         "alternate processes instead)")
    ap.add_argument("--steady-switch", default=None,
                    help="QE_SCORE_NARROW from the first run on (default: unset, the policy; -2: the policy without its probes; 0: single pass)")
    ap.add_argument("--cold-queued", action="store_true",
                    help="also: rounds of queued runs that start from unknown data and are never fetched -- the verdict is taken "
                         "when a run's counts reach the host, so such a stream keeps the first pass")
    ap.add_argument("--reseed", type=int, default=0, help="K > 0: a stream over K resident batches of different seeds per error rate")
    ap.add_argument("--schedule", default=None, help="with --reseed: error:runs,error:runs,... (default: --error for 24 runs)")
    ap.add_argument("--lib", default=None, help="with --reseed: the libquicked_hip.so to time (default: this tree's)")
    ap.add_argument("--out")
    args = ap.parse_args()
    os.environ.pop("QE_SCORE_NARROW", None)
    os.environ.pop("QUICKED_HIP_LIB", None)
    if args.reseed > 0:
        return reseeded(args)

    from bounded_bench import load_package
    from quicked_amd import capi, datagen
    batch = datagen.generate(args.count, args.length, args.error, seed=args.seed)
    kw = dict(algo=capi.BANDED, only_score=True, bandwidth=args.bandwidth)
    rb = capi.ResidentBatch(batch)
    params = capi.make_params(**kw)

    def switch(v):
        if v is None:
            os.environ.pop("QE_SCORE_NARROW", None)
        else:
            os.environ["QE_SCORE_NARROW"] = v
        capi.reload_env()

    def sync_run(b, p):
        t0 = time.perf_counter()
        if b.run(p, sync=True) < 0:
            raise RuntimeError("quicked_batch_run failed")
        return (time.perf_counter() - t0) * 1e3

    def round_of(b, p, steps):
        b.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            if b.run(p, sync=False) < 0:
                raise RuntimeError("quicked_batch_run failed")
        b.sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    prb = pp = None
    if args.parent:
        pcapi = load_package(os.path.abspath(args.parent), "parent_quicked_amd")
        prb = pcapi.ResidentBatch(batch)
        pp = pcapi.make_params(**kw)

    # warm-up: every set of the rotation, both launch sequences, neither touching the policy
    for v in ("1", "0"):
        switch(v)
        sync_run(rb, params)
        for _ in range(2):
            round_of(rb, params, args.steps)
    if prb:
        sync_run(prb, pp)
        for _ in range(2):
            round_of(prb, pp, args.steps)

    out = dict(only=args.only, pairs=args.count, length=args.length, error=args.error, bandwidth=args.bandwidth, rounds=args.rounds,
               steps_per_round=args.steps, unit="ms per run")
    # the first run on unknown data, against single-pass runs
    switch("0")
    single = [sync_run(rb, params) for _ in range(3)]
    single_scores = rb.scores()[0].copy()
    single_adv = int(rb.counters()[0])
    switch(args.steady_switch)              # (changing a switch has the library forget its verdicts: unknown data from here)
    first = sync_run(rb, params)
    c = rb.counters()
    out["first_run"] = dict(this_first_pass_ms=round(first, 4), this_single_pass_ms=stats(single), block_columns=int(c[0]),
                            second_pass_tasks=int(c[7]), single_pass_block_columns=single_adv)
    assert (rb.scores()[0] == single_scores).all(), "the two-pass run's scores differ from the single pass's"
    if prb:
        out["first_run"]["parent_ms"] = stats([sync_run(prb, pp) for _ in range(3)])
        assert (prb.scores()[0] == single_scores).all(), "scores differ from the parent's"

    # steady state
    times = {"this": [], "parent": []}
    for _ in range(args.rounds):
        if args.only != "parent":
            times["this"].append(round_of(rb, params, args.steps))
        if prb and args.only != "this":
            times["parent"].append(round_of(prb, pp, args.steps))
    out["steady"] = {k: stats(v) for k, v in times.items() if v}
    sync_run(rb, params)
    c = rb.counters()
    out["steady"]["block_columns_of_a_run_after"] = int(c[0])
    out["steady"]["second_pass_tasks_of_a_run_after"] = int(c[7])
    assert (rb.scores()[0] == single_scores).all()
    if args.cold_queued:
        capi.reload_env()                   # forget the verdicts
        cold = [round_of(rb, params, args.steps) for _ in range(args.rounds)]
        if rb.fetch() < 0:
            raise RuntimeError("quicked_batch_fetch failed")
        c = rb.counters()
        out["cold_queued"] = dict(this=stats(cold), block_columns_of_the_last_run=int(c[0]), second_pass_tasks_of_the_last_run=int(c[7]))
        assert (rb.scores()[0] == single_scores).all()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    rb.close()
    if prb:
        prb.close()


if __name__ == "__main__":
    main()
