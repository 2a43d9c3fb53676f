#!/usr/bin/env python3
"""All-occurrences panel runs (quicked_batch_run_panel_all): what they cost next to the routes the library offered before them.

    python tools/panel_hits_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_hits.json

The procedure of tools/search_panel_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max;
the ways of a leg alternate round by round, and every way brings its answers into numpy arrays inside the timed stretch.
    a   100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 4, max_hits 6 (the largest cap the pair batch admits:
        (tasks) x max_hits <= 2^26); every text holds one member with 8 % of
        its bases substituted.  run_panel_all against the 9.6 M-pair batch through quicked_batch_run_search_all with the same
        max_hits, regrouped per text in numpy.  The two routes must agree on every count and every field of every stored
        occurrence before anything is timed.
    b   run_panel_all alone at 1 000 000 such texts with max_hits 16: the sync call, the kernels (quicked_batch_kernel_times slot 0) and ps per
        block step (over quicked_batch_counters()[0]) -- next to the same ratio of run_panel (k_search_panel) on the same texts and
        of run_search_all in its register form (k_search_hits) on leg a of tools/search_bench.py (1 M pairs, 150 in 400, 4 %,
        bound 12, INFIX), all measured in the same process
    c   (--parent) the unflagged run_panel on leg a's texts and run_search_all on leg a of tools/search_bench.py, the parent
        commit's library and this one alternating: the new kernels share a translation unit and the scan's source with both
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
K, M, LENGTH, BOUND, MAX_HITS = 96, 24, 150, 4, 16
PAIRS_MAX_HITS = 6      # leg a: the largest cap the 9.6 M-pair batch admits ((tasks) x max_hits <= 2^26), used on both routes


def panel_all_answers(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    return found.astype(np.int64), off, np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64)


def regroup_pairs(rb, n, k, cap):
    """the pair batch's lists (pair i K + p: member p against text i) -> (found per text, text offsets, records): the pairs of a
    text are in member order and each pair's list is ordered by text_end, so a text's first `cap` are the first `cap` rows"""
    found, off, hits = rb.hits()
    counts = np.diff(off)
    pattern = np.repeat(np.arange(n * k, dtype=np.int64) % k, counts)
    rows = np.stack([pattern, hits["text_start"], hits["text_end"], hits["score"]], axis=1).astype(np.int64)
    per_text = counts.reshape(n, k).sum(axis=1)
    toff = np.concatenate([[0], np.cumsum(per_text)])
    keep = np.arange(len(rows)) - np.repeat(toff[:-1], per_text) < cap
    kept = np.minimum(per_text, cap)
    return found.reshape(n, k).sum(axis=1).astype(np.int64), np.concatenate([[0], np.cumsum(kept)]), rows[keep]


def leg_a(capi, datagen, rounds, n):
    panel, texts = SPB.make_set(n, K, M, LENGTH, 0.08, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    rq = capi.ResidentBatch(SPB.pair_batch(panel, texts, datagen))

    def panel_way():
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_INFIX, members, BOUND, max_hits=PAIRS_MAX_HITS) == capi.QUICKED_OK
        panel_way.out = panel_all_answers(rb)
        return float(rb.kernel_times()[0][0])

    def pair_way():
        rq.kernel_times()
        assert rq.run_search_all(capi.SEARCH_INFIX, BOUND, max_hits=PAIRS_MAX_HITS) == capi.QUICKED_OK
        pair_way.out = regroup_pairs(rq, n, K, PAIRS_MAX_HITS)
        return float(rq.kernel_times()[0][0])

    panel_way()
    pair_way()
    for a, b, what in zip(panel_way.out, pair_way.out, ("found", "offsets", "records")):
        assert a.shape == b.shape and (a == b).all(), f"leg a: the two routes differ in their {what}"
    found = panel_way.out[0]
    out = dict(leg="a", texts=n, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=PAIRS_MAX_HITS, mode="infix",
               occurrences=int(found.sum()), texts_with_two_or_more=int((found >= 2).sum()), texts_with_none=int((found == 0).sum()),
               ways=SPB.timed({"panel_all": panel_way, "pairs": pair_way}, rounds))
    out["panel_all_against_pairs"] = SPB.verdict(out["ways"]["panel_all"]["wall_ms"], out["ways"]["pairs"]["wall_ms"])
    out["panel_all_against_pairs_kernel"] = SPB.verdict(out["ways"]["panel_all"]["kernel_ms"], out["ways"]["pairs"]["kernel_ms"])
    rb.close()
    rq.close()
    return out


def search_leg(datagen, count):
    import search_bench
    leg = dict(search_bench.LEGS["a"])
    if count:
        leg["count"] = count
    base = datagen.generate(leg["count"], leg["m"], leg["error"], seed=leg["seed"])
    return leg, search_bench.embed(base, leg["n"], leg["seed"] + 1000, datagen)


def leg_b(capi, datagen, rounds, n, count_search):
    panel, texts = SPB.make_set(n, K, M, LENGTH, 0.08, 32)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    steps = {}

    def panel_all_way():
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        panel_all_answers(rb)
        steps["panel_all"] = int(rb.counters()[0])
        return float(rb.kernel_times()[0][0])

    def panel_all_prefix_way():                                    # PREFIX has no start pass: the forward kernel alone
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_PREFIX, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        panel_all_answers(rb)
        steps["panel_all_prefix"] = int(rb.counters()[0])
        return float(rb.kernel_times()[0][0])

    def panel_way():
        rb.kernel_times()
        assert rb.run_panel(capi.SEARCH_INFIX, members, BOUND) == capi.QUICKED_OK
        rb.panel_results()
        steps["panel"] = int(rb.counters()[0])
        return float(rb.kernel_times()[0][0])

    out = dict(leg="b", texts=n, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, mode="infix",
               ways=SPB.timed({"panel_all": panel_all_way, "panel_all_prefix": panel_all_prefix_way, "panel": panel_way}, rounds))
    rb.close()
    leg, batch = search_leg(datagen, count_search)
    rs = capi.ResidentBatch(batch)

    def hits_way():
        rs.kernel_times()
        assert rs.run_search_all(capi.SEARCH_INFIX, leg["bound"], max_hits=MAX_HITS) == capi.QUICKED_OK
        rs.hits()
        steps["search_all_registers"] = int(rs.counters()[0])
        return float(rs.kernel_times()[0][0])

    os.environ["QE_SEARCH_FORM"] = "1"
    capi.reload_env()
    out["ways"].update(SPB.timed({"search_all_registers": hits_way}, rounds))
    os.environ.pop("QE_SEARCH_FORM", None)
    capi.reload_env()
    rs.close()
    out["block_steps"] = dict(steps)
    out["ps_per_block_step"] = {w: round(out["ways"][w]["kernel_ms"]["median"] * 1e9 / steps[w], 3) for w in steps}
    return out


def leg_c(capi, pcapi, datagen, rounds, n, count_search):
    panel, texts = SPB.make_set(n, K, M, LENGTH, 0.08, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    tb = SPB.text_batch(texts, datagen)
    leg, sbatch = search_leg(datagen, count_search)
    libs = {"parent": pcapi, "this": capi}
    rbs = {name: (c, c.ResidentBatch(tb), c.ResidentBatch(sbatch)) for name, c in libs.items()}
    answers = {}

    def panel_way(name):
        c, rb, _ = rbs[name]

        def fn():
            rb.kernel_times()
            assert rb.run_panel(c.SEARCH_INFIX, members, BOUND) == c.QUICKED_OK
            answers["panel", name] = SPB.panel_answers(rb)
            return float(rb.kernel_times()[0][0])
        return fn

    def hits_way(name):
        c, _, rs = rbs[name]

        def fn():
            rs.kernel_times()
            assert rs.run_search_all(c.SEARCH_INFIX, leg["bound"], max_hits=MAX_HITS) == c.QUICKED_OK
            found, off, hits = rs.hits()
            answers["hits", name] = (found, off, np.stack([hits[f] for f in ("text_start", "text_end", "score")], axis=1))
            return float(rs.kernel_times()[0][0])
        return fn

    out = dict(leg="c", texts=n, members=K, pairs=leg["count"], pattern=leg["m"], text=leg["n"], search_bound=leg["bound"], mode="infix",
               ways=SPB.timed({"panel_parent": panel_way("parent"), "panel_this": panel_way("this")}, rounds))
    out["ways"].update(SPB.timed({"search_all_parent": hits_way("parent"), "search_all_this": hits_way("this")}, rounds))
    assert (answers["panel", "this"] == answers["panel", "parent"]).all()
    assert all((a == b).all() for a, b in zip(answers["hits", "this"], answers["hits", "parent"]))
    for run in ("panel", "search_all"):
        for what in ("wall_ms", "kernel_ms"):
            out[f"{run}_this_against_parent_{what}"] = SPB.verdict(out["ways"][run + "_this"][what], out["ways"][run + "_parent"][what])
    for _, rb, rs in rbs.values():
        rb.close()
        rs.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# All-occurrences panel runs: what was measured", "",
             f"`python tools/panel_hits_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays (for the pair route: the",
             "regrouping per text too).  *kernels*: `quicked_batch_kernel_times` slot 0, the search passes alone.  A way is called ahead",
             "or behind only where the medians differ by more than the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] == "a":
            lines += [f"## a: {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, bound {leg['bound']}, max_hits {leg['max_hits']}", "",
                      f"The two routes agreed on every count and every field of every stored occurrence ({leg['occurrences']} occurrences; "
                      f"{leg['texts_with_two_or_more']} texts with two or more, {leg['texts_with_none']} with none).", "",
                      "| route | sync call | kernels |", "|---|---|---|", row("run_panel_all", leg["ways"]["panel_all"]),
                      row(f"{leg['texts'] * leg['members']}-pair batch through run_search_all + numpy regrouping", leg["ways"]["pairs"]), "",
                      f"run_panel_all is **{leg['panel_all_against_pairs']}** on the sync call and **{leg['panel_all_against_pairs_kernel']}** on the kernels.  "
                      f"The pair batch was resident before the timing: its upload and its {leg['members']} copies of every text in HBM are not in these figures.", ""]
        elif leg["leg"] == "b":
            lines += [f"## b: per block step, {leg['texts']} texts x {leg['members']} members", "", "| run | sync call | kernels | block steps | ps per block step |", "|---|---|---|---|---|"]
            for w, label in (("panel_all", "run_panel_all, INFIX (k_panel_hits + the start pass)"), ("panel_all_prefix", "run_panel_all, PREFIX (k_panel_hits alone)"),
                             ("panel", "run_panel, INFIX (k_search_panel + the start pass)"),
                             ("search_all_registers", "run_search_all, register form (k_search_hits + the start pass; search leg a)")):
                lines.append(row(label, leg["ways"][w]) + f" {leg['block_steps'][w]} | {leg['ps_per_block_step'][w]} |")
            lines += ["", "The figure to measure against is k_search_hits' rate of this session (the last row), not a constant.", ""]
        elif leg["leg"] == "c":
            lines += [f"## c: the runs that existed, parent commit against this one (run_panel: {leg['texts']} texts x {leg['members']} members; run_search_all: {leg['pairs']} pairs, {leg['pattern']} in {leg['text']}, bound {leg['search_bound']})", "",
                      "| run, library | sync call | kernels |", "|---|---|---|"]
            for w in ("panel_parent", "panel_this", "search_all_parent", "search_all_this"):
                lines.append(row(w.replace("_", " "), leg["ways"][w]))
            lines += ["", f"run_panel: this commit is **{leg['panel_this_against_parent_wall_ms']}** with its parent on the sync call and **{leg['panel_this_against_parent_kernel_ms']}** on the kernels.  "
                      f"run_search_all: **{leg['search_all_this_against_parent_wall_ms']}** on the sync call and **{leg['search_all_this_against_parent_kernel_ms']}** on the kernels.", ""]
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
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    s = args.scale
    small = 0 if s >= 1 else max(64, int(1_000_000 * s))
    legs = []
    for leg in args.legs:
        if leg == "a":
            legs.append(leg_a(capi, datagen, args.rounds, max(64, int(100_000 * s))))
        elif leg == "b":
            legs.append(leg_b(capi, datagen, args.rounds, max(64, int(1_000_000 * s)), small))
        elif leg == "c" and args.parent:
            pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "PANEL_OCC_DTYPE"), "--parent must be a tree without all-occurrences panel runs"
            legs.append(leg_c(capi, pcapi, datagen, args.rounds, max(64, int(100_000 * s)), small))
        else:
            continue
        print(json.dumps(legs[-1]), flush=True)
    out = dict(unit="ms", rounds=args.rounds, scale=s, session=time.strftime("%Y-%m-%d"), legs=legs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
