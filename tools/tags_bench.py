#!/usr/bin/env python3
"""What alignment tags cost and what QUICKED_TAG_NO_CIGAR saves: QUICKED runs with sync != 0, so the clock includes the
results reaching the host.

    python tools/tags_bench.py --parent <tree of the parent commit, built> [--rounds 7] --out profiles/align_tags.json

Workloads: 100 000 pairs of 10 kb at 5 %, and 12 500 such pairs.  Legs, ms per run:
    p   the parent commit, CIGAR run (its library is loaded next to this tree's from its own folder)
    0   this tree, tags 0
    s   QUICKED_TAG_STATS
    m   QUICKED_TAG_STATS | QUICKED_TAG_MD
    n   QUICKED_TAG_STATS | QUICKED_TAG_NO_CIGAR
The legs alternate round by round in one process; one warm-up round is dropped; min / median / max over the rounds.  Before
the timing every leg's scores must agree, and the tag legs' statistics with each other.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [dict(count=100_000, length=10_000, error=0.05, seed=21), dict(count=12_500, length=10_000, error=0.05, seed=22)]
LEGS = {"0": dict(), "s": dict(stats=True), "m": dict(stats=True, md=True), "n": dict(stats=True, cigar=False)}


def load_package(tree, name):
    """the quicked_amd package of another tree under another module name (its capi binds its own library)"""
    path = os.path.join(tree, "quicked_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


def measure(capi, pcapi, datagen, w, rounds):
    batch = datagen.generate(w["count"], w["length"], w["error"], seed=w["seed"])
    rb = capi.ResidentBatch(batch)
    p = capi.make_params(algo=capi.QUICKED)
    forms = {}
    if pcapi:
        prb = pcapi.ResidentBatch(batch)
        pp = pcapi.make_params(algo=pcapi.QUICKED)
        forms["p"] = lambda: prb.run(pp, sync=True)

    def leg(tags):
        def run():
            if rb.configure_tags(**tags) < 0:
                raise RuntimeError("quicked_batch_configure_tags failed")
            return rb.run(p, sync=True)
        return run
    for k, tags in LEGS.items():
        forms[k] = leg(tags)

    # the same answers first
    ref_scores = ref_stats = None
    host_bytes = {}
    for k, f in forms.items():
        if f() < 0:
            raise RuntimeError(f"leg {k}: the run failed")
        scores = (prb if k == "p" else rb).scores()[0]
        if ref_scores is None:
            ref_scores = scores
        assert (scores == ref_scores).all(), f"leg {k}: scores differ on {int((scores != ref_scores).sum())} pairs"
        if k in "smn":
            st = rb.pair_stats()
            if ref_stats is None:
                ref_stats = st
            assert (st == ref_stats).all() and (st[:, 1] + st[:, 2] + st[:, 3] == scores).all(), f"leg {k}: statistics"
        if k != "p":
            lib, h = rb._lib, rb._h
            host_bytes[k] = dict(cigar=int(lib.quicked_batch_cigar_bytes(h)), md=int(lib.quicked_batch_md_bytes(h)),
                                 stats=32 * rb.n if k in "smn" else 0)
    times = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, f in forms.items():
            t0 = time.perf_counter()
            if f() < 0:
                raise RuntimeError(f"leg {k}: the run failed")
            dt = time.perf_counter() - t0
            if rnd > 0:                                  # round 0 warms pools, streams and clocks up
                times[k].append(dt * 1e3)
    out = dict(pairs=w["count"], length=w["length"], error=w["error"], host_bytes=host_bytes, legs={})
    for k, v in times.items():
        out["legs"][k] = dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3),
                              malign_per_s=round(w["count"] / statistics.median(v) / 1e3, 3), samples=[round(x, 3) for x in v])
    med = {k: statistics.median(v) for k, v in times.items()}
    out["ratios"] = {"s/0": round(med["s"] / med["0"], 4), "m/0": round(med["m"] / med["0"], 4)}
    if "p" in med:
        out["ratios"].update({"0/p": round(med["0"] / med["p"], 4), "n/p": round(med["n"] / med["p"], 4)})
        out["p_spread_ms"] = round(max(times["p"]) - min(times["p"]), 3)
        out["0_minus_p_ms"] = round(med["0"] - med["p"], 3)
    rb.close()
    if pcapi:
        prb.close()
    return out


def markdown(out):
    """the figures as a short table per workload (written next to --out)"""
    names = {"p": "(p) parent, CIGAR run", "0": "(0) tags 0", "s": "(s) STATS", "m": "(m) STATS + MD", "n": "(n) STATS + NO_CIGAR"}
    lines = ["# Alignment tags: QUICKED sync runs, results on the host", "",
             f"`python tools/tags_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}`; ms per run, "
             "min / median / max over the rounds after a warm-up round, the legs alternating in one process.", ""]
    for w in out["workloads"]:
        lines += [f"## {w['pairs']} pairs of {w['length']} at {w['error']:.0%}", "", "| leg | min | median | max | M alignments/s | bytes to the host: CIGAR / MD / stats |", "|---|---|---|---|---|---|"]
        for k, v in w["legs"].items():
            hb = w["host_bytes"].get(k)
            lines.append(f"| {names[k]} | {v['min']} | {v['median']} | {v['max']} | {v['malign_per_s']} | " +
                         (f"{hb['cigar']} / {hb['md']} / {hb['stats']} |" if hb else "|"))
        r = w["ratios"]
        lines += ["", "Ratios of medians: " + ", ".join(f"{k} = {v}" for k, v in r.items()) + "."]
        if "p_spread_ms" in w:
            lines.append(f"(0) - (p) = {w['0_minus_p_ms']} ms; (p)'s own rounds spread over {w['p_spread_ms']} ms (max - min).")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no p leg)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--count", type=int, nargs="*", help="override the workloads' numbers of pairs (smoke runs)")
    ap.add_argument("--length", type=int, default=0, help="override the read length")
    ap.add_argument("--out")
    args = ap.parse_args()
    for name in ("QE_TAGS_WAVE", "QE_FORMAT_WAVE", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    pcapi = None
    if args.parent:
        pcapi = load_package(os.path.abspath(args.parent), "parent_quicked_amd")
        assert "quicked_batch_configure_tags" not in pcapi.EXPORTS, "--parent must be a tree without the tags"
    workloads = [dict(w) for w in WORKLOADS]
    if args.count:
        workloads = [dict(WORKLOADS[0], count=c) for c in args.count]
    if args.length:
        for w in workloads:
            w["length"] = args.length
    out = dict(unit="ms per sync run (QUICKED, results on the host)", rounds=args.rounds, workloads=[])
    for w in workloads:
        out["workloads"].append(measure(capi, pcapi, datagen, w, args.rounds))
        print(json.dumps(out["workloads"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
