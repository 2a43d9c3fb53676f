#!/usr/bin/env python3
"""Occurrence alignments (QUICKED_PANEL_CIGARS): what they cost next to the run without them and next to the pair route.

    python tools/panel_cigars_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_cigars.json

The procedure of tools/panel_hits_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max;
the ways of a leg alternate round by round, and every way brings its answers into numpy arrays / Python objects inside the
timed stretch.
    a   100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 4, max_hits 6; every text holds one member with 8 % of
        its bases substituted.  Three ways: run_panel_all with the bit (records + strings), run_panel_all without it (records),
        and the pair route -- the run without the bit, the stretches cut out on the host, a (member, stretch) pair batch created
        and run through run_bounded(bound = score) with CIGARs.  The strings of the first and the third are asserted identical
        before anything is timed.  The alignment pass (quicked_batch_kernel_times slot 1) per occurrence and per block step
        (quicked_batch_counters()[1]) next to the search passes' ps per block step (slot 0 over counter [0]) of the same run.
    b   the same with 96 members of 200 bases in texts of 1 000 (bound 8): four-block histories and sub-batches; and one text
        of 5 Mb through run_panel_scan (24-base members, bound 2), with and without the bit.
    c   (--parent) run_panel_all, run_panel_scan and run_panel without the bit on leg a's texts, the parent commit's library and
        this one alternating.
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
K, BOUND, MAX_HITS = 96, 4, 6


def records(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    return found.astype(np.int64), off, np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64)


def pair_route(capi, datagen, rb, members, texts, length, bound, max_hits):
    """the run without the bit, the host cut-out, a pair batch and run_bounded with CIGARs -> (records, strings)"""
    assert rb.run_panel_all(capi.SEARCH_INFIX, members, bound, max_hits=max_hits) == capi.QUICKED_OK
    found, off, rows = records(rb)
    text_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    m = len(members[0])
    flat = ACGT[texts].reshape(-1)
    lens = (rows[:, 2] - rows[:, 1]).astype(np.int32)
    toff = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64) if len(lens) else np.zeros(0, dtype=np.int64)
    src = np.repeat(text_of * length + rows[:, 1] - toff, lens) + np.arange(int(lens.sum()))
    tp = np.concatenate([flat[src], np.zeros(1, dtype=np.uint8)])
    pp = np.concatenate([np.frombuffer(b"".join(members), dtype=np.uint8).reshape(len(members), m)[rows[:, 0]].reshape(-1), np.zeros(1, dtype=np.uint8)])
    rq = capi.ResidentBatch(datagen.PairBatch(pp, np.arange(len(rows), dtype=np.int64) * m, np.full(len(rows), m, dtype=np.int32), tp, toff, lens))
    assert rq.run_bounded(rows[:, 3].astype(np.int32), only_score=False) >= 0
    cig = rq.cigars()
    rq.close()
    return (found, off, rows), cig


def cigar_leg(capi, datagen, rounds, n, m, length, bound, max_hits, seed, name, with_pairs):
    panel, texts = SPB.make_set(n, K, m, length, 0.08, seed)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    info = {}

    def flagged():
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_INFIX | capi.PANEL_CIGARS, members, bound, max_hits=max_hits) == capi.QUICKED_OK
        flagged.out = (records(rb), rb.panel_hit_cigars())
        ms, launches = rb.kernel_times()
        c = rb.counters()
        info.update(search_steps=int(c[0]), align_steps=int(c[1]), operations=int(c[3]), align_launches=int(launches[1]))
        info.setdefault("align_ms", []).append(float(ms[1]))
        return float(ms[0])

    def plain():
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_INFIX, members, bound, max_hits=max_hits) == capi.QUICKED_OK
        plain.out = records(rb)
        return float(rb.kernel_times()[0][0])

    def pairs():
        pairs.out = pair_route(capi, datagen, rb, members, texts, length, bound, max_hits)
        return None

    ways = {"flagged": flagged, "plain": plain}
    flagged()
    plain()
    assert all((a == b).all() for a, b in zip(flagged.out[0], plain.out)), f"leg {name}: the bit changed the records"
    if with_pairs:
        pairs()
        assert all((a == b).all() for a, b in zip(flagged.out[0], pairs.out[0]))
        assert flagged.out[1] == pairs.out[1], f"leg {name}: the two routes' strings differ"
        ways["pairs"] = pairs
    info["align_ms"] = []
    nocc = int(flagged.out[0][1][-1])
    out = dict(leg=name, texts=n, members=K, member_bases=m, text_bases=length, bound=bound, max_hits=max_hits, mode="infix", occurrences=nocc,
               example=flagged.out[1][:3], ways=SPB.timed(ways, rounds))
    align = SPB.stat(info["align_ms"][1:])                            # (the first timed call is the warm-up round's)
    out["align_pass"] = dict(kernel_ms=align, launches=info["align_launches"], block_steps=info["align_steps"], operations=info["operations"],
                             ns_per_occurrence=round(align["median"] * 1e6 / max(nocc, 1), 3),
                             ps_per_block_step=round(align["median"] * 1e9 / max(info["align_steps"], 1), 3))
    out["search_passes"] = dict(block_steps=info["search_steps"],
                                ps_per_block_step=round(out["ways"]["flagged"]["kernel_ms"]["median"] * 1e9 / max(info["search_steps"], 1), 3))
    out["flagged_against_plain"] = SPB.verdict(out["ways"]["flagged"]["wall_ms"], out["ways"]["plain"]["wall_ms"])
    if with_pairs:
        out["flagged_against_pairs"] = SPB.verdict(out["ways"]["flagged"]["wall_ms"], out["ways"]["pairs"]["wall_ms"])
    rb.close()
    return out


def scan_leg(capi, datagen, rounds, bases):
    rng = np.random.default_rng(77)
    panel = rng.integers(0, 4, (K, 24), dtype=np.uint8)
    text = rng.integers(0, 4, (1, bases), dtype=np.uint8)
    for at in range(1000, bases - 100, 2500):                          # a member every 2.5 kb, every third with a substituted base
        q = panel[(at // 2500) % K].copy()
        if (at // 2500) % 3 == 0:
            q[11] = (q[11] + 1) % 4
        text[0, at:at + 24] = q
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(text, datagen))
    info = {}

    def way(bit):
        def fn():
            rb.kernel_times()
            assert rb.run_panel_scan(capi.SEARCH_INFIX | bit, members, 2, max_hits=4096) == capi.QUICKED_OK
            fn.out = records(rb)
            if bit:
                fn.cig = rb.panel_hit_cigars()
            ms, launches = rb.kernel_times()
            if bit:
                info.setdefault("align_ms", []).append(float(ms[1]))
                info["align_steps"] = int(rb.counters()[1])
            return float(ms[0])
        return fn

    flagged, plain = way(capi.PANEL_CIGARS), way(0)
    out = dict(leg="b_scan", text_bases=bases, members=K, member_bases=24, bound=2, max_hits=4096, ways=SPB.timed({"flagged": flagged, "plain": plain}, rounds))
    assert all((a == b).all() for a, b in zip(flagged.out, plain.out))
    nocc = int(flagged.out[1][-1])
    align = SPB.stat(info["align_ms"][1:])
    out.update(occurrences=nocc, example=flagged.cig[:3], flagged_against_plain=SPB.verdict(out["ways"]["flagged"]["wall_ms"], out["ways"]["plain"]["wall_ms"]),
               align_pass=dict(kernel_ms=align, block_steps=info["align_steps"], ns_per_occurrence=round(align["median"] * 1e6 / max(nocc, 1), 3)))
    rb.close()
    return out


def leg_c(capi, pcapi, datagen, rounds, n):
    panel, texts = SPB.make_set(n, K, 24, 150, 0.08, 31)
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
            elif run == "panel_scan":
                assert rb.run_panel_scan(c.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
                answers[run, name] = records(rb)
            else:
                assert rb.run_panel(c.SEARCH_INFIX, members, BOUND) == c.QUICKED_OK
                answers[run, name] = (SPB.panel_answers(rb),)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="c", texts=n, members=K, member_bases=24, text_bases=150, bound=BOUND, max_hits=MAX_HITS, ways={})
    for run in ("panel_all", "panel_scan", "panel"):
        out["ways"].update(SPB.timed({f"{run}_parent": way(run, "parent"), f"{run}_this": way(run, "this")}, rounds))
        assert all((a == b).all() for a, b in zip(answers[run, "this"], answers[run, "parent"])), run
        for what in ("wall_ms", "kernel_ms"):
            out[f"{run}_this_against_parent_{what}"] = SPB.verdict(out["ways"][run + "_this"][what], out["ways"][run + "_parent"][what])
    for _, rb in rbs.values():
        rb.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# Occurrence alignments (QUICKED_PANEL_CIGARS): what was measured", "",
             f"`python tools/panel_cigars_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + (f", text counts scaled by {out['scale']}" if out["scale"] != 1 else "") +
             ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays and Python strings (for the",
             "pair route: the cut-out, the pair batch's creation and upload, run_bounded and its getter too).  *kernels*:",
             "`quicked_batch_kernel_times` slot 0, the search passes alone; the alignment pass is slot 1.  A way is called ahead or behind",
             "only where the medians differ by more than the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] in ("a", "b"):
            a = leg["align_pass"]
            lines += [f"## {leg['leg']}: {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, bound {leg['bound']}, max_hits {leg['max_hits']}", "",
                      f"{leg['occurrences']} stored occurrences; the first strings: {', '.join(leg['example'])}.", "",
                      "| way | sync call | kernels (slot 0) |", "|---|---|---|", row("run_panel_all with the bit: records + strings", leg["ways"]["flagged"]),
                      row("run_panel_all without it: records", leg["ways"]["plain"])]
            if "pairs" in leg["ways"]:
                lines.append(row("pair route: the run without the bit, host cut-out, pair batch, run_bounded with CIGARs", leg["ways"]["pairs"]))
            lines += ["", f"The flagged run is **{leg['flagged_against_plain']}** the run without the bit" +
                      (f" and **{leg['flagged_against_pairs']}** against the pair route (sync call); the two routes' strings were identical, all {leg['occurrences']} of them." if "flagged_against_pairs" in leg else " (sync call)."), "",
                      f"The alignment pass: {a['kernel_ms']['min']} / {a['kernel_ms']['median']} / {a['kernel_ms']['max']} ms in {a['launches']} launch(es), "
                      f"{a['block_steps']} block steps, {a['operations']} operations: **{a['ns_per_occurrence']} ns per occurrence, {a['ps_per_block_step']} ps per block step**, "
                      f"next to the search passes' {leg['search_passes']['ps_per_block_step']} ps per block step ({leg['search_passes']['block_steps']} steps) in the same runs.", ""]
        elif leg["leg"] == "b_scan":
            a = leg["align_pass"]
            lines += [f"## b, one text of {leg['text_bases']} bases through run_panel_scan x {leg['members']} members of {leg['member_bases']}, bound {leg['bound']}", "",
                      f"{leg['occurrences']} stored occurrences; the first strings: {', '.join(leg['example'])}.", "",
                      "| way | sync call | kernels (slot 0) |", "|---|---|---|", row("with the bit", leg["ways"]["flagged"]), row("without it", leg["ways"]["plain"]), "",
                      f"The flagged run is **{leg['flagged_against_plain']}** the run without the bit (sync call).  The alignment pass: {a['kernel_ms']['median']} ms, {a['ns_per_occurrence']} ns per occurrence.", ""]
        elif leg["leg"] == "c":
            lines += [f"## c: the runs without the bit, parent commit against this one ({leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, bound {leg['bound']}, max_hits {leg['max_hits']})", "",
                      "| run, library | sync call | kernels |", "|---|---|---|"]
            for run in ("panel_all", "panel_scan", "panel"):
                for lib in ("parent", "this"):
                    lines.append(row(f"run_{run}, {lib}", leg["ways"][f"{run}_{lib}"]))
            lines += [""] + [f"run_{run}: this commit is **{leg[run + '_this_against_parent_wall_ms']}** with its parent on the sync call and **{leg[run + '_this_against_parent_kernel_ms']}** on the kernels."
                             for run in ("panel_all", "panel_scan", "panel")] + [""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no leg c)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", nargs="*", default=["a", "b", "c"])
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
            legs.append(cigar_leg(capi, datagen, args.rounds, max(64, int(100_000 * s)), 24, 150, BOUND, MAX_HITS, 31, "a", True))
        elif leg == "b":
            legs.append(cigar_leg(capi, datagen, args.rounds, max(64, int(100_000 * s)), 200, 1000, 8, MAX_HITS, 33, "b", False))
            print(json.dumps(legs[-1]), flush=True)
            legs.append(scan_leg(capi, datagen, args.rounds, max(20_000, int(5_000_000 * s))))
        elif leg == "c" and args.parent:
            pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "PANEL_CIGARS"), "--parent must be a tree without occurrence alignments"
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
