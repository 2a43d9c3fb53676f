#!/usr/bin/env python3
"""The windowed mismatch-only panel run (quicked_batch_run_panel_scan_no_indels): what splitting long texts across lanes buys
under QUICKED_PANEL_NO_INDELS, which window it wants, what it costs where there is nothing to split, and whether the routes that
existed before are untouched.

    python tools/panel_noindels_scan_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_noindels_scan.json

The procedure of tools/panel_scan_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max; the
ways of a leg alternate round by round, and every way brings its answers into numpy arrays inside the timed stretch.
    a   1 text of 5 Mb, and 8 texts of 5 Mb, x 96 members of 24 bases, INFIX, bound 2, max_hits 16; every 50 kb one member is
        planted with 8 % of its bases substituted.  run_panel_scan_no_indels (window 0) against run_panel_all | PANEL_NO_INDELS
        on the same batch -- the only route there was.  The two must agree on every array before anything is timed.  Per way:
        the sync call, the kernels (quicked_batch_kernel_times slot 0), ps per block step (over quicked_batch_counters()[0]);
        for the scan the share of its block steps that run_panel_all does not walk: lead-in and run-out starts
    b   the window sweep on both batches of leg a: forced windows of 1024 .. 65536 in powers of two, and the library's own
    c   one window per text: 100 000 texts of 150 bases x the same panel, the scan against the flagged run_panel_all
    d   (--parent) run_panel_scan, run_panel_all and run_panel, the last two flagged and unflagged, on leg c's texts: the parent
        commit's library and this one alternating, parent first
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import panel_scan_bench as PSB        # noqa: E402
import search_panel_bench as SPB      # noqa: E402

ACGT = SPB.ACGT
K, M, BOUND, MAX_HITS = PSB.K, PSB.M, 2, 16
SWEEP = PSB.SWEEP


def leg_ab(capi, datagen, rounds, count, length):
    members, tb = PSB.long_batch(datagen, count, length, 40 + count)
    rb = capi.ResidentBatch(tb)
    mode = capi.SEARCH_INFIX | capi.PANEL_NO_INDELS
    steps = {}

    def scan_way(window):
        def fn():
            rb.kernel_times()
            assert rb.run_panel_scan_no_indels(mode, members, BOUND, max_hits=MAX_HITS, window=window) == capi.QUICKED_OK
            fn.out = PSB.answers(rb)
            steps[fn.name] = int(rb.counters()[0])
            return float(rb.kernel_times()[0][0])
        fn.name = "scan" if window == 0 else f"scan_{window}"
        return fn

    def all_way():
        rb.kernel_times()
        assert rb.run_panel_all(mode, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        all_way.out = PSB.answers(rb)
        steps["panel_all"] = int(rb.counters()[0])
        return float(rb.kernel_times()[0][0])

    ways = {"scan": scan_way(0), "panel_all": all_way}
    sweep = {f"scan_{w}": scan_way(w) for w in SWEEP}
    all_way()
    for fn in list(sweep.values()) + [ways["scan"]]:
        fn()
        for a, b, what in zip(fn.out, all_way.out, ("found", "offsets", "records")):
            assert a.shape == b.shape and (a == b).all(), f"{fn.name}: differs from the flagged run_panel_all in its {what}"
    a = dict(leg="a", texts=count, text_bases=length, members=K, member_bases=M, bound=BOUND, max_hits=MAX_HITS, mode="infix, no indels",
             occurrences=int(all_way.out[0].sum()), library_window=PSB.library_window(count * length), ways=SPB.timed(ways, rounds))
    a["block_steps"] = {w: steps[w] for w in ways}
    a["ps_per_block_step"] = {w: round(a["ways"][w]["kernel_ms"]["median"] * 1e9 / steps[w], 3) for w in ways}
    a["scan_extra_step_share"] = round((steps["scan"] - steps["panel_all"]) / steps["scan"], 5)
    a["scan_against_panel_all"] = SPB.verdict(a["ways"]["scan"]["wall_ms"], a["ways"]["panel_all"]["wall_ms"])
    a["scan_against_panel_all_kernel"] = SPB.verdict(a["ways"]["scan"]["kernel_ms"], a["ways"]["panel_all"]["kernel_ms"])
    a["factor"] = round(a["ways"]["panel_all"]["wall_ms"]["median"] / a["ways"]["scan"]["wall_ms"]["median"], 1)
    b = dict(leg="b", texts=count, text_bases=length, library_window=a["library_window"], ways=SPB.timed(dict(sweep, scan=ways["scan"]), rounds))
    b["extra_step_share"] = {w: round((steps[w] - steps["panel_all"]) / steps[w], 5) for w in b["ways"]}
    rb.close()
    return a, b


def short_set(datagen, n):
    panel, texts = SPB.make_set(n, K, M, 150, 0.08, 31)
    return [ACGT[panel[p]].tobytes() for p in range(K)], SPB.text_batch(texts, datagen)


def leg_c(capi, datagen, rounds, n):
    members, tb = short_set(datagen, n)
    rb = capi.ResidentBatch(tb)
    mode = capi.SEARCH_INFIX | capi.PANEL_NO_INDELS

    def scan_way():
        rb.kernel_times()
        assert rb.run_panel_scan_no_indels(mode, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        scan_way.out = PSB.answers(rb)
        return float(rb.kernel_times()[0][0])

    def all_way():
        rb.kernel_times()
        assert rb.run_panel_all(mode, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        all_way.out = PSB.answers(rb)
        return float(rb.kernel_times()[0][0])

    scan_way()
    all_way()
    assert all(a.shape == b.shape and (a == b).all() for a, b in zip(scan_way.out, all_way.out))
    out = dict(leg="c", texts=n, text_bases=150, members=K, member_bases=M, bound=BOUND, max_hits=MAX_HITS, mode="infix, no indels",
               ways=SPB.timed({"scan": scan_way, "panel_all": all_way}, rounds))
    out["scan_against_panel_all"] = SPB.verdict(out["ways"]["scan"]["wall_ms"], out["ways"]["panel_all"]["wall_ms"])
    out["scan_against_panel_all_kernel"] = SPB.verdict(out["ways"]["scan"]["kernel_ms"], out["ways"]["panel_all"]["kernel_ms"])
    out["gap_ms"] = round(out["ways"]["scan"]["wall_ms"]["median"] - out["ways"]["panel_all"]["wall_ms"]["median"], 4)
    rb.close()
    return out


RUNS_D = ("panel_scan", "panel_all", "panel_all_noindels", "panel", "panel_noindels")


def leg_d(capi, pcapi, datagen, rounds, n):
    members, tb = short_set(datagen, n)
    rbs = {"parent": (pcapi, pcapi.ResidentBatch(tb)), "this": (capi, capi.ResidentBatch(tb))}
    got = {}

    def way(run, name):
        c, rb = rbs[name]
        ni = c.PANEL_NO_INDELS if run.endswith("noindels") else 0

        def fn():
            rb.kernel_times()
            if run == "panel_scan":
                assert rb.run_panel_scan(c.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
            elif run.startswith("panel_all"):
                assert rb.run_panel_all(c.SEARCH_INFIX | ni, members, BOUND, max_hits=MAX_HITS) == c.QUICKED_OK
            else:
                assert rb.run_panel(c.SEARCH_INFIX | ni, members, BOUND) == c.QUICKED_OK
            got[run, name] = (SPB.panel_answers(rb),) if run in ("panel", "panel_noindels") else PSB.answers(rb)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="d", texts=n, text_bases=150, members=K, mode="infix", ways={})
    for run in RUNS_D:
        out["ways"].update(SPB.timed({run + "_parent": way(run, "parent"), run + "_this": way(run, "this")}, rounds))      # parent first
        assert all((a == b).all() for a, b in zip(got[run, "this"], got[run, "parent"])), run
        for what in ("wall_ms", "kernel_ms"):
            out[f"{run}_this_against_parent_{what}"] = SPB.verdict(out["ways"][run + "_this"][what], out["ways"][run + "_parent"][what])
    for _, rb in rbs.values():
        rb.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# The windowed mismatch-only panel run: what was measured", "",
             f"`python tools/panel_noindels_scan_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays.  *kernels*:",
             "`quicked_batch_kernel_times` slot 0, the sweep alone (the count, offset, ranking and finish kernels are in the sync call only).",
             "A way is called ahead or behind only where the medians differ by more than the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] == "a":
            lines += [f"## a: {leg['texts']} text(s) of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, no indels, bound {leg['bound']}, max_hits {leg['max_hits']}", "",
                      f"Both runs agreed on every array ({leg['occurrences']} occurrences).  The library's window here: {leg['library_window']} columns.", "",
                      "| run | sync call | kernels | block steps | ps per block step |", "|---|---|---|---|---|"]
            for w, label in (("scan", "run_panel_scan_no_indels, window 0"), ("panel_all", "run_panel_all, PANEL_NO_INDELS (one lane per text)")):
                lines.append(row(label, leg["ways"][w]) + f" {leg['block_steps'][w]} | {leg['ps_per_block_step'][w]} |")
            lines += ["", f"run_panel_scan_no_indels is **{leg['scan_against_panel_all']}** on the sync call ({leg['factor']} times by the medians) and "
                      f"**{leg['scan_against_panel_all_kernel']}** on the kernels; {100 * leg['scan_extra_step_share']:.3f} % of its block steps are lead-in and run-out starts.", ""]
        elif leg["leg"] == "b":
            lines += [f"## b: the window sweep, {leg['texts']} text(s) of {leg['text_bases']} (the library's choice: {leg['library_window']})", "",
                      "| window | sync call | kernels | lead-in and run-out share of the block steps |", "|---|---|---|---|"]
            for w in leg["ways"]:
                lines.append(row("the library's" if w == "scan" else w.split("_")[1], leg["ways"][w]) + f" {100 * leg['extra_step_share'][w]:.3f} % |")
            lines.append("")
        elif leg["leg"] == "c":
            lines += [f"## c: one window per text, {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members, no indels", "", "| run | sync call | kernels |", "|---|---|---|",
                      row("run_panel_scan_no_indels, window 0", leg["ways"]["scan"]), row("run_panel_all, PANEL_NO_INDELS", leg["ways"]["panel_all"]), "",
                      f"run_panel_scan_no_indels is **{leg['scan_against_panel_all']}** on the sync call (median gap {leg['gap_ms']} ms: the slot table and the ranking pass) "
                      f"and **{leg['scan_against_panel_all_kernel']}** on the kernels.", ""]
        elif leg["leg"] == "d":
            lines += [f"## d: the runs that existed, parent commit against this one ({leg['texts']} texts of {leg['text_bases']} x {leg['members']} members)", "",
                      "| run, library | sync call | kernels |", "|---|---|---|"]
            for run in RUNS_D:
                for lib in ("parent", "this"):
                    lines.append(row(f"{run.replace('_', ' ')}, {lib}", leg["ways"][f"{run}_{lib}"]))
            lines.append("")
            for run in RUNS_D:
                lines.append(f"{run}: this commit is **{leg[run + '_this_against_parent_wall_ms']}** with its parent on the sync call and **{leg[run + '_this_against_parent_kernel_ms']}** on the kernels.  ")
            lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no leg d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", nargs="*", default=["a", "c", "d"], help="a brings b with it")
    ap.add_argument("--scale", type=float, default=1.0, help="scale the legs' sizes (smoke runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.rounds >= 7 or args.scale < 1, "medians of at least 7 rounds"
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    s = args.scale
    legs = []

    def done(leg):
        legs.append(leg)
        print(json.dumps(leg), flush=True)

    for leg in args.legs:
        if leg == "a":
            for count in (1, 8):
                a, b = leg_ab(capi, datagen, args.rounds, count, max(70_000, int(5_000_000 * s)))
                done(a)
                done(b)
        elif leg == "c":
            done(leg_c(capi, datagen, args.rounds, max(64, int(100_000 * s))))
        elif leg == "d" and args.parent:
            pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi.ResidentBatch, "run_panel_scan_no_indels"), "--parent must be a tree without the windowed mismatch-only run"
            done(leg_d(capi, pcapi, datagen, args.rounds, max(64, int(100_000 * s))))
    out = dict(unit="ms", rounds=args.rounds, scale=s, session=time.strftime("%Y-%m-%d"), legs=legs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                     # one line per leg
            head = json.dumps({k: v for k, v in out.items() if k != "legs"})
            f.write(head[:-1] + ', "legs": [\n' + ",\n".join(json.dumps(leg) for leg in legs) + "\n]}\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
