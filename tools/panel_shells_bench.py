#!/usr/bin/env python3
"""The seven per-text sweep kernels of panel search, both equalities: the parent commit's library against this one.

    python tools/panel_shells_bench.py --parent <built tree of the parent commit> [--runs 3] [--rounds 5] --out profiles/panel_shells.json

For a change that must leave the sweeps' time where it was (profiles/panel_shells.md).  One process; per kernel a batch that
both libraries hold, and `runs` runs of tools/search_panel_bench.py's timed(): one warm-up round, then `rounds` rounds in which
parent and this alternate.  The figure is quicked_batch_kernel_times slot 0 of the run that launches the kernel (with its start
pass, whose kernel is not a sweep).  Both libraries must give the same answers in every round.
    best / ham        run_panel, plain / PANEL_NO_INDELS                       100 000 texts of 150 x 96 members of 24, INFIX, bound 2
    hits / ham_hits   run_panel_all, plain / PANEL_NO_INDELS, max_hits 6       the same
    tails / heads     run_panel_all | PANEL_TAILS / | PANEL_HEADS              the same (heads: slot 0 holds k_panel_hits too)
    scan              run_panel_scan, the library's window                     16 texts of 500 000 x the same members
each under the library's equality and under SEARCH_IUPAC.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import search_panel_bench as SPB      # noqa: E402

K, M, BOUND, MAX_HITS = 96, 24, 2, 6


def fields(a):
    return np.stack([a[f] for f in a.dtype.names], axis=1).astype(np.int64)


def occurrences(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    return [found, stored, off, fields(hits)]


def runner(c, rb, kernel, eq, members):
    mode = c.SEARCH_INFIX | (c.SEARCH_IUPAC if eq else 0)

    def fn():
        rb.kernel_times()
        if kernel in ("best", "ham"):
            assert rb.run_panel(mode | (c.PANEL_NO_INDELS if kernel == "ham" else 0), members, BOUND) == c.QUICKED_OK
            fn.answers = [fields(rb.panel_results())]
        elif kernel == "scan":
            assert rb.run_panel_scan(mode, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
            fn.answers = occurrences(rb)
        else:
            bit = dict(hits=0, ham_hits=c.PANEL_NO_INDELS, tails=c.PANEL_TAILS, heads=c.PANEL_HEADS)[kernel]
            assert rb.run_panel_all(mode | bit, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
            fn.answers = occurrences(rb) + ([fields(rb.panel_tails())] if kernel == "tails" else []) + ([fields(rb.panel_heads())] if kernel == "heads" else [])
        return float(rb.kernel_times()[0][0])
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checked-out and built tree of the parent commit")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the text counts and lengths (smoke runs)")
    ap.add_argument("--kernels", nargs="*", default=["best", "hits", "tails", "heads", "ham", "ham_hits", "scan"])
    ap.add_argument("--out")
    args = ap.parse_args()
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
    libs = {"parent": pcapi, "this": capi}
    shapes = {"short": (max(64, int(100_000 * args.scale)), 150), "long": (16, max(4096, int(500_000 * args.scale)))}
    out = dict(unit="ms", runs=args.runs, rounds=args.rounds, scale=args.scale, kernels=[])
    for shape, (n, length) in shapes.items():
        mine = [k for k in args.kernels if (k == "scan") == (shape == "long")]
        if not mine:
            continue
        panel, texts = SPB.make_set(n, K, M, length, 0.08, 53)
        members = [SPB.ACGT[panel[p]].tobytes() for p in range(K)]
        tb = SPB.text_batch(texts, datagen)
        rbs = {lib: c.ResidentBatch(tb) for lib, c in libs.items()}
        for lib, rb in rbs.items():
            assert rb.configure_panel_tails(8) == libs[lib].QUICKED_OK and rb.configure_panel_heads(8) == libs[lib].QUICKED_OK
        for kernel in mine:
            for eq in (0, 1):
                ways = {lib: runner(libs[lib], rbs[lib], kernel, eq, members) for lib in libs}
                series = {lib: [] for lib in libs}
                for _ in range(args.runs):
                    t = SPB.timed(ways, args.rounds)
                    assert all((a == b).all() for a, b in zip(ways["this"].answers, ways["parent"].answers)), (kernel, eq)
                    for lib in libs:
                        series[lib].append(t[lib]["kernel_ms"])
                flat = {lib: [x for r in series[lib] for x in r["samples"]] for lib in libs}
                spread = round(max(flat["parent"]) - min(flat["parent"]), 4)
                gap = round(float(np.median(flat["this"]) - np.median(flat["parent"])), 4)
                row = dict(kernel=kernel, equality="iupac" if eq else "library", texts=n, text_bases=length,
                           parent_runs=[r["samples"] for r in series["parent"]], this_runs=[r["samples"] for r in series["this"]],
                           parent_median=round(float(np.median(flat["parent"])), 4), this_median=round(float(np.median(flat["this"])), 4),
                           parent_spread=spread, this_minus_parent=gap, within_parent_spread=bool(abs(gap) <= spread))
                out["kernels"].append(row)
                print(json.dumps(row), flush=True)
        for rb in rbs.values():
            rb.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{" + ",\n ".join(json.dumps(k) + ": " + json.dumps(v) for k, v in out.items()).replace('{"kernel"', '\n  {"kernel"') + "}\n")


if __name__ == "__main__":
    main()
