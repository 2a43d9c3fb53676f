#!/usr/bin/env python3
"""What the IUPAC equality of search runs costs: QUICKED_SEARCH_IUPAC / QUICKED_SEARCH_IUPAC_PATTERN against the unflagged run
on one upper-case ACGT batch, where all three give identical results (asserted before anything is timed).

    python tools/search_iupac_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/search_iupac.json
    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python tools/search_iupac_bench.py --trace-run
    python tools/search_iupac_bench.py --trace-stats <dir> --out profiles/search_iupac_pack.json

Shapes: 1 000 000 pairs of a 150-base pattern in a 400-base text at 4 %, bound 12 (legs a / c of profiles/search.md), and
BIG of tests/golden/make_search_cases.py (20 000 such pairs).  Each in INFIX and PREFIX, each in both kernel forms
(QE_SEARCH_FORM = 0 workspace, 1 registers).  Legs, interleaved round by round in one process, one warm-up round dropped:
    p    the parent commit's unflagged run (its library is loaded next to this tree's from its own folder)
    0    this tree, unflagged
    i    mode | QUICKED_SEARCH_IUPAC
    ip   mode | QUICKED_SEARCH_IUPAC_PATTERN
Per leg: the whole synchronous run (host clock around a sync != 0 call: results on the host) and the sweep alone
(quicked_batch_kernel_times slot 0: HIP events around the search passes; the pack launches of a flagged run are outside
them), min / median / max over the rounds.  Where the flagged sweep's median is behind the unflagged one's by more than the
larger of the two spreads the leg is marked.  --trace-run does a few flagged and unflagged runs of the first shape (ASCII, then packed PLANES3) and nothing
else, for a kernel trace of its own (no counters in that run); --trace-stats reads the trace's kernel statistics.
"""
import argparse
import csv
import glob
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"1M": dict(count=1_000_000, m=150, n=400, error=0.04, bound=12, seed=21), "BIG": None}
IUPAC, IUPAC_PATTERN = 16, 32


def load_package(tree, name):
    """the quicked_amd package of another tree under another module name (its capi binds its own library)"""
    path = os.path.join(tree, "quicked_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


def make_batch(name, datagen, count=0):
    if name == "BIG":
        spec = importlib.util.spec_from_file_location("make_search_cases", os.path.join(ROOT, "tests", "golden", "make_search_cases.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        pairs = mod.big_batch()[:count or None]
        pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
        tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
        po = np.concatenate([[0], np.cumsum(pl[:-1])]).astype(np.int64)
        to = np.concatenate([[0], np.cumsum(tl[:-1])]).astype(np.int64)
        batch = datagen.PairBatch(np.frombuffer(b"".join(p for p, _ in pairs), dtype=np.uint8).copy(), po, pl,
                                  np.frombuffer(b"".join(t for _, t in pairs), dtype=np.uint8).copy(), to, tl)
        return batch, mod.BIG["bound"], dict(pairs=len(pairs), pattern=mod.BIG["m"], text=mod.BIG["n"], error=mod.BIG["rate"])
    import search_bench
    s = dict(SHAPES[name])
    if count:
        s["count"] = count
    base = datagen.generate(s["count"], s["m"], s["error"], seed=s["seed"])
    return search_bench.embed(base, s["n"], s["seed"] + 1000, datagen), s["bound"], dict(pairs=s["count"], pattern=s["m"], text=s["n"], error=s["error"])


def set_form(capis, switch):
    os.environ["QE_SEARCH_FORM"] = switch
    for c in capis:
        c.reload_env()


def answers(rb):
    sc = rb.scores()[0]
    ts, te = rb.locations()
    return np.stack([sc, ts, te], axis=1)


def stat(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), spread=round(max(v) - min(v), 4),
                samples=[round(x, 4) for x in v])


def measure(name, capi, pcapi, datagen, rounds, count):
    batch, bound, desc = make_batch(name, datagen, count)
    rb = capi.ResidentBatch(batch)
    prb = pcapi.ResidentBatch(batch) if pcapi else None
    capis = [capi] + ([pcapi] if pcapi else [])
    out = dict(shape=name, bound=bound, **desc, runs=[])
    for mode_name, mode in (("infix", capi.SEARCH_INFIX), ("prefix", capi.SEARCH_PREFIX)):
        for form_name, switch in (("workspace", "0"), ("registers", "1")):
            set_form(capis, switch)
            legs = {}
            if prb:
                legs["p"] = (prb, mode)
            legs.update({"0": (rb, mode), "i": (rb, mode | IUPAC), "ip": (rb, mode | IUPAC_PATTERN)})
            # identical results first: ACGT input
            ref = None
            for k, (b, md) in legs.items():
                if b.run_search(md, bound, only_score=True, sync=True) < 0:
                    raise RuntimeError(f"leg {k}: the run failed")
                a = answers(b)
                ref = a if ref is None else ref
                assert (a == ref).all(), f"{name} {mode_name} {form_name}: leg {k} differs on {int((a != ref).any(axis=1).sum())} pairs"
            wall = {k: [] for k in legs}
            sweep = {k: [] for k in legs}
            steps = {}
            for rnd in range(rounds + 1):
                for k, (b, md) in legs.items():
                    b.kernel_times()
                    t0 = time.perf_counter()
                    if b.run_search(md, bound, only_score=True, sync=True) < 0:
                        raise RuntimeError(f"leg {k}: the run failed")
                    dt = time.perf_counter() - t0
                    ms, _ = b.kernel_times()
                    steps[k] = int(b.counters()[0])
                    if rnd > 0:                              # round 0 warms pools, streams and clocks up
                        wall[k].append(dt * 1e3)
                        sweep[k].append(float(ms[0]))
            assert len(set(steps.values())) == 1, steps      # the same block steps under every equality
            run = dict(mode=mode_name, form=form_name, within=int((ref[:, 0] >= 0).sum()), block_steps=steps["0"],
                       sync_run_ms={k: stat(v) for k, v in wall.items()}, sweep_ms={k: stat(v) for k, v in sweep.items()})
            s0 = run["sweep_ms"]["0"]
            for k in ("i", "ip"):
                sk = run["sweep_ms"][k]
                run[f"sweep_{k}_minus_0_ms"] = round(sk["median"] - s0["median"], 4)
                run[f"sweep_{k}_behind"] = bool(sk["median"] - s0["median"] > max(sk["spread"], s0["spread"]))
                run[f"sync_run_{k}_minus_0_ms"] = round(run["sync_run_ms"][k]["median"] - run["sync_run_ms"]["0"]["median"], 4)
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.environ.pop("QE_SEARCH_FORM", None)
    for c in capis:
        c.reload_env()
    rb.close()
    if prb:
        prb.close()
    return out


def markdown(out):
    names = {"p": "parent, unflagged", "0": "unflagged", "i": "IUPAC", "ip": "IUPAC_PATTERN"}
    lines = ["# Search runs under the IUPAC equality: what was measured", "",
             f"`python tools/search_iupac_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X.  One upper-case ACGT",
             "batch per shape, device-resident; every leg gave identical scores and locations before the timing.  The legs alternate",
             "round by round in one process, one warm-up round dropped; ms, min / median / max.  *sync run*: host clock around one",
             "`sync != 0` call, results on the host.  *sweep*: `quicked_batch_kernel_times` slot 0, the search passes alone (the",
             "pack launches of a flagged run are not in it).", ""]
    for w in out["shapes"]:
        lines += [f"## {w['pairs']} pairs, pattern {w['pattern']} in text {w['text']}, {w['error']:.0%}, bound {w['bound']}", ""]
        for r in w["runs"]:
            lines += [f"### {r['mode'].upper()}, {r['form']} form ({r['block_steps']} block steps, {r['within']} pairs within the bound)", "",
                      "| leg | sync run | sweep |", "|---|---|---|"]
            for k in r["sync_run_ms"]:
                a, b = r["sync_run_ms"][k], r["sweep_ms"][k]
                lines.append(f"| {names[k]} | {a['min']} / {a['median']} / {a['max']} | {b['min']} / {b['median']} / {b['max']} |")
            lines += ["", "Sweep, flagged - unflagged medians: " + ", ".join(
                f"{names[k]} {r[f'sweep_{k}_minus_0_ms']:+} ms" + (" (**behind** by more than the larger spread)" if r[f"sweep_{k}_behind"] else "")
                for k in ("i", "ip")) + ".  Sync run: " + ", ".join(f"{names[k]} {r[f'sync_run_{k}_minus_0_ms']:+} ms" for k in ("i", "ip")) + ".", ""]
    return "\n".join(lines)


def trace_run(capi, datagen, count):
    """a few runs of the first shape, flagged and not, INFIX (both pack directions), as an ASCII and as a packed PLANES3 batch,
    for rocprofv3 --kernel-trace --stats"""
    batch, bound, _ = make_batch("1M", datagen, count)
    rb = capi.ResidentBatch(batch)
    for _ in range(4):
        for md in (capi.SEARCH_INFIX, capi.SEARCH_INFIX | IUPAC, capi.SEARCH_INFIX | IUPAC_PATTERN):
            if rb.run_search(md, bound, only_score=True, sync=True) < 0:
                raise RuntimeError("the run failed")
    rb.close()
    # the same pairs as a packed batch: its flagged runs derive the four planes from the resident three (k_planes_iupac)
    rk = capi.ResidentBatch(batch, wire=capi.WIRE_PLANES3)
    for _ in range(4):
        for md in (capi.SEARCH_INFIX | IUPAC, capi.SEARCH_INFIX | IUPAC_PATTERN):
            if rk.run_search(md, bound, only_score=True, sync=True) < 0:
                raise RuntimeError("the packed run failed")
    rk.close()
    print("trace run ok")


def trace_stats(directory):
    """-> per kernel of interest {calls, total_ms, mean_us} from rocprofv3's kernel statistics"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                n = row.get("Name", "")
                if "k_pack" in n or "k_planes_iupac" in n or "k_search" in n or "k_reverse_planes" in n:
                    calls = int(row["Calls"])
                    total = float(row.get("TotalDurationNs") or row["TotalDuration"])
                    e = out.setdefault(n, dict(calls=0, total_ms=0.0))
                    e["calls"] += calls
                    e["total_ms"] = round(e["total_ms"] + total / 1e6, 4)
    for e in out.values():
        e["mean_us"] = round(e["total_ms"] * 1e3 / max(1, e["calls"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no p leg)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--count", type=int, default=0, help="override the shapes' numbers of pairs (smoke runs)")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-stats", help="directory of a rocprofv3 --kernel-trace --stats run of --trace-run")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.rounds >= 7 or args.count, "medians of at least 7 rounds"
    if args.trace_stats:
        out = dict(unit="per launch, from one rocprofv3 --kernel-trace --stats run of --trace-run (no counters)", kernels=trace_stats(args.trace_stats))
    else:
        for name in ("QE_SEARCH_FORM", "QUICKED_HIP_LIB"):
            os.environ.pop(name, None)
        from quicked_amd import capi, datagen
        if args.trace_run:
            trace_run(capi, datagen, args.count)
            return
        pcapi = None
        if args.parent:
            pcapi = load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "SEARCH_IUPAC"), "--parent must be a tree without the flags"
        out = dict(unit="ms", rounds=args.rounds, shapes=[measure(n, capi, pcapi, datagen, args.rounds, args.count) for n in args.shapes])
    print(json.dumps(out if args.trace_stats else {"done": len(out["shapes"])}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        if not args.trace_stats:
            with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
                f.write(markdown(out))


if __name__ == "__main__":
    main()
