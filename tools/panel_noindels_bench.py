#!/usr/bin/env python3
"""Mismatch-only panel runs (QUICKED_PANEL_NO_INDELS): what the flagged runs take, and whether the runs without the bit moved.

    python tools/panel_noindels_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_noindels.json

The procedure of tools/panel_heads_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max;
the ways of a leg alternate round by round, and every way brings its answers into numpy arrays inside the timed stretch.
    a   100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 2, max_hits 6, every text holding one member with 8 %
        of its bases substituted.  Four ways on the same batch: run_panel and run_panel_all with the bit, and the same two
        without it -- as context only: they answer another question.  Whole-run time, quicked_batch_kernel_times slot 0, the
        block steps (counter [0]) and the kernels' ps per block step.
    p   the same, PREFIX.
    m   1 000 000 texts x the same 96 members, INFIX.
    k   2 000 texts x 4 096 members, INFIX.
    c   (--parent) run_panel and run_panel_all WITHOUT the bit on leg a's texts, the parent commit's library and this one
        alternating.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import search_panel_bench as SPB      # noqa: E402

ACGT = SPB.ACGT
OCC_FIELDS = ("pattern", "text_start", "text_end", "score")
M, LENGTH, BOUND, MAX_HITS = 24, 150, 2, 6


def records(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    return found.astype(np.int64), off, np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64)


def leg_bit(capi, datagen, rounds, n, k, name, base):
    """legs a, p, m and k: both runs with the bit and, beside them, without it"""
    panel, texts = SPB.make_set(n, k, M, LENGTH, 0.08, 47)
    members = [ACGT[panel[p]].tobytes() for p in range(k)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    steps, answers = {}, {}

    def way(run, bit):
        def fn():
            rb.kernel_times()
            if run == "panel_all":
                assert rb.run_panel_all(base | bit, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
                answers[run, bit] = records(rb)
            else:
                assert rb.run_panel(base | bit, members, BOUND) == capi.QUICKED_OK
                answers[run, bit] = (SPB.panel_answers(rb),)
            steps[run, bit] = int(rb.counters()[0])
            return float(rb.kernel_times()[0][0])
        return fn

    NI = capi.PANEL_NO_INDELS
    ways = {"panel_flagged": way("panel", NI), "panel_all_flagged": way("panel_all", NI), "panel_plain": way("panel", 0), "panel_all_plain": way("panel_all", 0)}
    out = dict(leg=name, texts=n, members=k, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, mode="infix" if base == capi.SEARCH_INFIX else "prefix",
               ways=SPB.timed(ways, rounds))
    starts = (LENGTH - M + 1) if base == capi.SEARCH_INFIX else 1
    assert steps["panel", NI] == steps["panel_all", NI] == n * k * starts, "counter [0] of a flagged run is texts x members x starts x blocks"
    best = answers["panel", NI][0]
    out.update(flagged_block_steps=steps["panel", NI], plain_panel_block_steps=steps["panel", 0], plain_panel_all_block_steps=steps["panel_all", 0],
               flagged_texts_with_a_member=int((np.asarray(best)[:, 0] >= 0).sum()), flagged_occurrences=int(answers["panel_all", NI][1][-1]),
               plain_occurrences=int(answers["panel_all", 0][1][-1]))
    for w, key in (("panel_flagged", ("panel", NI)), ("panel_all_flagged", ("panel_all", NI)), ("panel_plain", ("panel", 0)), ("panel_all_plain", ("panel_all", 0))):
        out[w + "_ps_per_block_step"] = round(out["ways"][w]["kernel_ms"]["median"] * 1e9 / max(steps[key], 1), 3)
    rb.close()
    return out


def leg_c(capi, pcapi, datagen, rounds, n, k):
    panel, texts = SPB.make_set(n, k, M, LENGTH, 0.08, 47)
    members = [ACGT[panel[p]].tobytes() for p in range(k)]
    tb = SPB.text_batch(texts, datagen)
    rbs = {"parent": (pcapi, pcapi.ResidentBatch(tb)), "this": (capi, capi.ResidentBatch(tb))}
    answers = {}

    def way(run, name):
        c, rb = rbs[name]

        def fn():
            rb.kernel_times()
            if run == "panel_all":
                assert rb.run_panel_all(c.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
                answers[run, name] = records(rb)
            else:
                assert rb.run_panel(c.SEARCH_INFIX, members, BOUND) == c.QUICKED_OK
                answers[run, name] = (SPB.panel_answers(rb),)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="c", texts=n, members=k, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, ways={})
    for run in ("panel_all", "panel"):
        out["ways"].update(SPB.timed({f"{run}_parent": way(run, "parent"), f"{run}_this": way(run, "this")}, rounds))
        assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(answers[run, "this"], answers[run, "parent"])), run
        for what in ("wall_ms", "kernel_ms"):
            out[f"{run}_this_against_parent_{what}"] = SPB.verdict(out["ways"][run + "_this"][what], out["ways"][run + "_parent"][what])
    for _, rb in rbs.values():
        rb.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# Mismatch-only panel runs (QUICKED_PANEL_NO_INDELS): what was measured", "",
             f"`python tools/panel_noindels_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + (f", text counts scaled by {out['scale']}" if out["scale"] != 1 else "") +
             ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays.  *kernels*:",
             "`quicked_batch_kernel_times` slot 0.  A way is called ahead or behind only where the medians differ by more than the larger",
             "of the two spreads (DESIGN.md 4.9), else level.  The runs without the bit stand beside the flagged ones as context only:",
             "they answer another question (edit distance), stop a member early once it has an exact answer, and add a start pass.", ""]
    for leg in out["legs"]:
        if leg["leg"] != "c":
            lines += [f"## {leg['leg']}: {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, {leg['mode'].upper()}, bound {leg['bound']}, max_hits {leg['max_hits']}", "",
                      f"{leg['flagged_texts_with_a_member']} texts have a member within {leg['bound']} mismatches; {leg['flagged_occurrences']} stored occurrences with the bit, {leg['plain_occurrences']} without.", "",
                      "| way | sync call | kernels (slot 0) | block steps | ps per block step |", "|---|---|---|---|---|"]
            for w, label, steps in (("panel_flagged", "run_panel, the bit", "flagged_block_steps"), ("panel_all_flagged", "run_panel_all, the bit", "flagged_block_steps"),
                                    ("panel_plain", "run_panel, no bit", "plain_panel_block_steps"), ("panel_all_plain", "run_panel_all, no bit", "plain_panel_all_block_steps")):
                lines.append(row(label, leg["ways"][w]) + f" {leg[steps]} | {leg[w + '_ps_per_block_step']} |")
            lines.append("")
        else:
            lines += [f"## c: the runs without the bit, parent commit against this one ({leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, bound {leg['bound']}, max_hits {leg['max_hits']})", "",
                      "| run, library | sync call | kernels |", "|---|---|---|"]
            for run in ("panel_all", "panel"):
                for lib in ("parent", "this"):
                    lines.append(row(f"run_{run}, {lib}", leg["ways"][f"{run}_{lib}"]))
            lines += [""] + [f"run_{run}: this commit is **{leg[run + '_this_against_parent_wall_ms']}** with its parent on the sync call and **{leg[run + '_this_against_parent_kernel_ms']}** on the kernels."
                             for run in ("panel_all", "panel")] + [""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no leg c)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", nargs="*", default=["a", "p", "m", "k", "c"])
    ap.add_argument("--scale", type=float, default=1.0, help="scale the legs' text counts (smoke runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.rounds >= 7 or args.scale < 1, "medians of at least 7 rounds"
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    s = args.scale
    legs = []
    for leg in args.legs:
        if leg == "a":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(100_000 * s)), 96, "a", capi.SEARCH_INFIX))
        elif leg == "p":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(100_000 * s)), 96, "p", capi.SEARCH_PREFIX))
        elif leg == "m":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(1_000_000 * s)), 96, "m", capi.SEARCH_INFIX))
        elif leg == "k":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(2_000 * s)), 4096, "k", capi.SEARCH_INFIX))
        elif leg == "c" and args.parent:
            pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "PANEL_NO_INDELS"), "--parent must be a tree without the bit"
            legs.append(leg_c(capi, pcapi, datagen, args.rounds, max(64, int(100_000 * s)), 96))
        else:
            continue
        print(json.dumps(legs[-1]), flush=True)
    out = dict(unit="ms", rounds=args.rounds, scale=s, session=time.strftime("%Y-%m-%d"), legs=legs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{" + ",\n ".join(json.dumps(k) + ": " + json.dumps(v) for k, v in out.items()).replace('{"leg"', '\n  {"leg"') + "}\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
