#!/usr/bin/env python3
"""5' heads (QUICKED_PANEL_HEADS): what the bit costs next to the run without it, and whether the runs without it moved.

    python tools/panel_heads_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_heads.json

The procedure of tools/panel_tails_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max;
the ways of a leg alternate round by round, and every way brings its answers into numpy arrays inside the timed stretch.
    a   the README's panel workload -- 100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 4, max_hits 6, every
        text holding one member with 8 % of its bases substituted -- with a third of the texts beginning with the last 8 .. 20
        bases of a member.  Two ways on the same batch: run_panel_all with the bit (records + heads) and without it (records).
        The records are asserted identical before anything is timed.  Whole-run time and quicked_batch_kernel_times slot 0 (the
        forward kernel, the head kernels and the start / end passes), the head sweep's block steps (counter [6]) and its walk's
        row steps (counter [7]) next to the occurrences' block steps (counter [0]).
    b   the same batch, TAILS | HEADS against TAILS: records and tails asserted identical first.
    l   10 000 texts of 10 000 bases x the same 96 members, a third beginning inside a member, the bit against no bit.
    c   (--parent) run_panel_all and run_panel without the bit on leg a's texts, the parent commit's library and this one
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
TAIL_FIELDS = ("pattern", "overlap", "text_start", "score")
HEAD_FIELDS = ("pattern", "overlap", "text_end", "score")
K, M, LENGTH, BOUND, MAX_HITS = 96, 24, 150, 4, 6


def make_set(n, seed, length=LENGTH):
    """SPB.make_set's texts, every third beginning with the last 8 .. 20 bases of a member -> (panel, texts, member or -1, bases)"""
    panel, texts = SPB.make_set(n, K, M, length, 0.08, seed)
    rng = np.random.default_rng(seed + 1)
    which = np.where(np.arange(n) % 3 == 0, rng.integers(0, K, n), -1)
    bases = rng.integers(8, 21, n)
    for i in np.nonzero(which >= 0)[0]:
        texts[i, :bases[i]] = panel[which[i], M - bases[i]:]
    return panel, texts, which, bases


def records(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    return found.astype(np.int64), off, np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64)


def tails(rb):
    t = rb.panel_tails()
    return np.stack([t[f] for f in TAIL_FIELDS], axis=1).astype(np.int64)


def heads(rb):
    t = rb.panel_heads()
    return np.stack([t[f] for f in HEAD_FIELDS], axis=1).astype(np.int64)


def leg_bit(capi, datagen, rounds, n, name, length, beside):
    """legs a, b and l: the mode `beside` (0 or PANEL_TAILS) with the bit against the same mode without it"""
    panel, texts, which, bases = make_set(n, 31, length)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    info = {}
    mode = capi.SEARCH_INFIX | beside

    def answers():
        return records(rb) + ((tails(rb),) if beside else ())

    def flagged():
        rb.kernel_times()
        assert rb.run_panel_all(mode | capi.PANEL_HEADS, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        flagged.out = (answers(), heads(rb))
        c = rb.counters()
        info.update(block_steps=int(c[0]), head_block_steps=int(c[6]), head_row_steps=int(c[7]))
        return float(rb.kernel_times()[0][0])

    def plain():
        rb.kernel_times()
        assert rb.run_panel_all(mode, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        plain.out = answers()
        return float(rb.kernel_times()[0][0])

    flagged()
    plain()
    assert all((a == b).all() for a, b in zip(flagged.out[0], plain.out)), "the bit changed the records"
    t = flagged.out[1]
    planted = which >= 0
    # a planted suffix of r bases is a head of its member at r or more matched bases (a longer chance extension may win)
    assert (t[planted, 0] >= 0).all() and ((t[planted, 1] - t[planted, 3]) >= bases[planted]).all() and (t[planted, 2] >= 0).all()
    out = dict(leg=name, texts=n, members=K, member_bases=M, text_bases=length, bound=BOUND, max_hits=MAX_HITS, mode="infix", min_overlap=3,
               beside="tails" if beside else "none", occurrences=int(flagged.out[0][1][-1]), planted=int(planted.sum()),
               texts_with_a_head=int((t[:, 0] >= 0).sum()), planted_member_reported=int((t[planted, 0] == which[planted]).sum()),
               ways=SPB.timed({"flagged": flagged, "plain": plain}, rounds))
    out.update(info)
    out.update(head_block_steps_per_block_step=round(info["head_block_steps"] / max(info["block_steps"], 1), 4))
    for what in ("wall_ms", "kernel_ms"):
        f, p = out["ways"]["flagged"][what], out["ways"]["plain"][what]
        out[f"flagged_against_plain_{what}"] = SPB.verdict(f, p)
        out[f"flagged_over_plain_{what}"] = round(f["median"] / p["median"], 4)
    rb.close()
    return out


def leg_c(capi, pcapi, datagen, rounds, n):
    panel, texts, _, _ = make_set(n, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
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

    out = dict(leg="c", texts=n, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, ways={})
    for run in ("panel_all", "panel"):
        out["ways"].update(SPB.timed({f"{run}_parent": way(run, "parent"), f"{run}_this": way(run, "this")}, rounds))
        assert all((a == b).all() for a, b in zip(answers[run, "this"], answers[run, "parent"])), run
        for what in ("wall_ms", "kernel_ms"):
            out[f"{run}_this_against_parent_{what}"] = SPB.verdict(out["ways"][run + "_this"][what], out["ways"][run + "_parent"][what])
    for _, rb in rbs.values():
        rb.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# 5' heads (QUICKED_PANEL_HEADS): what was measured", "",
             f"`python tools/panel_heads_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + (f", text counts scaled by {out['scale']}" if out["scale"] != 1 else "") +
             ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays.  *kernels*:",
             "`quicked_batch_kernel_times` slot 0: the forward kernel, the head kernels and the start / end passes.  A way is called ahead or",
             "behind only where the medians differ by more than the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] in ("a", "b", "l"):
            with_, without = ("TAILS + HEADS", "TAILS") if leg["beside"] == "tails" else ("the bit", "no bit")
            lines += [f"## {leg['leg']}: {with_} against {without}, {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, bound {leg['bound']}, max_hits {leg['max_hits']}, min_overlap {leg['min_overlap']}", "",
                      f"{leg['planted']} texts begin with the last 8 .. 20 bases of a member; {leg['texts_with_a_head']} texts have a head, {leg['planted_member_reported']} of the planted",
                      f"ones report the planted member (the others a member with an equal or better key); {leg['occurrences']} stored occurrences, the same with and without the bit.", "",
                      "| way | sync call | kernels (slot 0) |", "|---|---|---|", row(f"run_panel_all, {with_}", leg["ways"]["flagged"]),
                      row(f"run_panel_all, {without}", leg["ways"]["plain"]), "",
                      f"The flagged run is **{leg['flagged_against_plain_wall_ms']}** the run without the bit on the sync call ({leg['flagged_over_plain_wall_ms']} x) and "
                      f"**{leg['flagged_against_plain_kernel_ms']}** on the kernels ({leg['flagged_over_plain_kernel_ms']} x).  The head sweep took {leg['head_block_steps']} block steps "
                      f"and its walk {leg['head_row_steps']} row steps beside the occurrences' {leg['block_steps']} block steps ({leg['head_block_steps_per_block_step']} per block step).", ""]
        elif leg["leg"] == "c":
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
    ap.add_argument("--legs", nargs="*", default=["a", "b", "l", "c"])
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
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(100_000 * s)), "a", LENGTH, 0))
        elif leg == "b":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(100_000 * s)), "b", LENGTH, capi.PANEL_TAILS))
        elif leg == "l":
            legs.append(leg_bit(capi, datagen, args.rounds, max(64, int(10_000 * s)), "l", 10_000, 0))
        elif leg == "c" and args.parent:
            pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "PANEL_HEADS"), "--parent must be a tree without the heads"
            legs.append(leg_c(capi, pcapi, datagen, args.rounds, max(64, int(100_000 * s))))
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
