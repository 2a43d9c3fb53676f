#!/usr/bin/env python3
"""Bounded runs against the two ways there were to get the same answers: the diagonal-word form (k_bounded_diag), the
general path (QE_BOUNDED_DIAG=0: the BandEd score pass with the bound as cutoff), and -- the baseline -- the cheapest
call of a tree WITHOUT the mode: quicked_batch_run BANDED only_score at bandwidth 1, thresholded by the caller.

    python tools/bounded_bench.py --leg a --parent <tree of the parent commit, built> [--rounds 7] [--steps 8] --out profiles/bounded_a.json

Legs (device-resident batch, queued runs timed as bench.py's headline does: `steps` runs with sync=False, one sync):
    a   100 000 pairs of 10 kb, 0.3 % planted edits, bound 48    (parent: cutoff 100)
    b   1 000 000 pairs of 150 b, 2 %, bound 8                   (parent: the band geometry's floor of 65)
The three forms alternate round by round in one process (the parent's library is loaded next to this tree's from its
own folder and uses only calls it has); one warm-up round is dropped; min / median / max over the rounds are reported,
and the three must give the same within / beyond answers on the timed inputs.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"a": dict(count=100_000, length=10_000, error=0.003, bound=48, seed=11),
        "b": dict(count=1_000_000, length=150, error=0.02, bound=8, seed=12)}


def load_package(tree, name):
    """the quicked_amd package of another tree under another module name (its capi binds its own library)"""
    path = os.path.join(tree, "quicked_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), required=True)
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no baseline leg)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--count", type=int, default=0, help="override the leg's number of pairs (smoke runs)")
    ap.add_argument("--length", type=int, default=0, help="override the leg's read length (where does the default choice turn?)")
    ap.add_argument("--bound", type=int, default=-1, help="override the leg's bound")
    ap.add_argument("--out")
    args = ap.parse_args()
    leg = dict(LEGS[args.leg])
    if args.count:
        leg["count"] = args.count
    if args.length:
        leg["length"] = args.length
    if args.bound >= 0:
        leg["bound"] = args.bound
    os.environ.pop("QE_BOUNDED_DIAG", None)
    os.environ.pop("QUICKED_HIP_LIB", None)

    from quicked_amd import capi, datagen
    batch = datagen.generate(leg["count"], leg["length"], leg["error"], seed=leg["seed"])
    bound = leg["bound"]
    rb = capi.ResidentBatch(batch)
    forms = {}

    def bounded(switch):
        def prepare():
            os.environ["QE_BOUNDED_DIAG"] = switch
            capi.reload_env()

        def step():
            if rb.run_bounded(bound, only_score=True, sync=False) < 0:
                raise RuntimeError("quicked_batch_run_bounded failed")

        def answers():
            prepare()
            rb.kernel_times()
            assert rb.run_bounded(bound, only_score=True, sync=True) >= 0
            _, launches = rb.kernel_times()
            assert (launches[3] > 0) == (switch == "1"), (switch, launches)
            return rb.scores()[0]
        return dict(prepare=prepare, step=step, sync=rb.sync, answers=answers)

    forms["diag"] = bounded("1")
    forms["general"] = bounded("0")
    if args.parent:
        pcapi = load_package(os.path.abspath(args.parent), "parent_quicked_amd")
        assert "quicked_batch_run_bounded" not in pcapi.EXPORTS, "--parent must be a tree without the mode"
        prb = pcapi.ResidentBatch(batch)
        pp = pcapi.make_params(algo=pcapi.BANDED, only_score=True, bandwidth=1)

        def pstep():
            if prb.run(pp, sync=False) < 0:
                raise RuntimeError("parent: quicked_batch_run failed")

        def panswers():
            assert prb.run(pp, sync=True) >= 0
            s = prb.scores()[0]
            return np.where((s >= 0) & (s <= bound), s, -1)
        forms["parent_banded_bw1"] = dict(prepare=lambda: None, step=pstep, sync=prb.sync, answers=panswers)

    # the same answers first
    ans = {k: f["answers"]() for k, f in forms.items()}
    ref = ans["diag"]
    for k, a in ans.items():
        assert (a == ref).all(), f"{k} disagrees with diag on {int((a != ref).sum())} pairs"
    within = int((ref >= 0).sum())

    times = {k: [] for k in forms}
    for rnd in range(args.rounds + 1):
        for k, f in forms.items():
            f["prepare"]()
            f["sync"]()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f["step"]()
            f["sync"]()
            dt = (time.perf_counter() - t0) / args.steps
            if rnd > 0:                              # round 0 warms pools, streams and clocks up
                times[k].append(dt * 1e3)
    out = dict(leg=args.leg, pairs=leg["count"], length=leg["length"], error=leg["error"], bound=bound, within=within,
               rounds=args.rounds, steps_per_round=args.steps, unit="ms per queued run", forms={})
    for k, v in times.items():
        out["forms"][k] = dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4),
                               malign_per_s=round(leg["count"] / statistics.median(v) / 1e3, 3), samples=[round(x, 4) for x in v])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
