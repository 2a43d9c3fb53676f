#!/usr/bin/env python3
"""Panel runs (quicked_batch_run_panel): what they cost next to the only route the library offered before them.

    python tools/search_panel_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/search_panel.json

Legs; medians of `rounds` rounds after one warm-up round, with min and max; the ways of a leg alternate round by round in
one process, and every way brings its answers into numpy arrays inside the timed stretch:
    a   100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 4; every text holds one member with 8 % of its bases
        substituted.  The panel run against the 9.6 M-pair batch through quicked_batch_run_search with the reduction by the key
        (score, panel index) in numpy.  The two routes must agree on every field of every text before anything is timed.
    b   the panel run alone at 1 000 000 such texts: the sync call, the kernels (quicked_batch_kernel_times slot 0) and ps per
        block step (over quicked_batch_counters()[0]) -- next to the same ratio of k_search in both its forms on leg a of
        tools/search_bench.py (1 M pairs, 150 in 400, 4 %, bound 12, INFIX), measured in the same process
    c   2 000 texts of 150 bases x 4096 members of 24 bases: QE_PANEL_SLICES=1 against the host's choice
    d   (--parent) the unflagged best search on leg a of tools/search_bench.py, the parent commit's library and this one
        alternating: the panel kernels share a translation unit with k_search
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
HIT_FIELDS = ("pattern", "score", "text_start", "text_end", "second_pattern", "second_score")


def load_package(tree, name):
    """the quicked_amd package of another tree under another module name (its capi binds its own library)"""
    path = os.path.join(tree, "quicked_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


def stat(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), spread=round(max(v) - min(v), 4),
                samples=[round(x, 4) for x in v])


def verdict(a, b):
    """a against b by the rule of DESIGN.md 4.9: ahead / behind only where the medians differ by more than the larger spread"""
    gap = b["median"] - a["median"]
    if abs(gap) <= max(a["spread"], b["spread"]):
        return "level"
    return "ahead" if gap > 0 else "behind"


def make_set(n, k, m, length, rate, seed):
    """-> (panel codes [k, m], text codes [n, length]): every text random, one member planted with `rate` of its bases substituted"""
    rng = np.random.default_rng(seed)
    panel = rng.integers(0, 4, (k, m), dtype=np.uint8)
    texts = rng.integers(0, 4, (n, length), dtype=np.uint8)
    which = rng.integers(0, k, n)
    planted = panel[which]
    sub = rng.random((n, m)) < rate
    planted = np.where(sub, (planted + rng.integers(1, 4, (n, m), dtype=np.uint8)) % 4, planted).astype(np.uint8)
    at = rng.integers(0, length - m + 1, n)
    texts[np.arange(n)[:, None], at[:, None] + np.arange(m)[None, :]] = planted
    return panel, texts


def text_batch(texts, datagen):
    n, length = texts.shape
    none = np.zeros(1, dtype=np.uint8)
    return datagen.PairBatch(none, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), ACGT[texts].reshape(-1),
                             np.arange(n, dtype=np.int64) * length, np.full(n, length, dtype=np.int32))


def pair_batch(panel, texts, datagen):
    """the n x K pair batch: pair i K + p is member p against text i"""
    (k, m), (n, length) = panel.shape, texts.shape
    pp = np.tile(ACGT[panel].reshape(-1), n)
    tp = np.repeat(ACGT[texts], k, axis=0).reshape(-1)
    return datagen.PairBatch(pp, np.arange(n * k, dtype=np.int64) * m, np.full(n * k, m, dtype=np.int32), tp,
                             np.arange(n * k, dtype=np.int64) * length, np.full(n * k, length, dtype=np.int32))


def panel_answers(rb):
    r = rb.panel_results()
    return np.stack([r[f] for f in HIT_FIELDS], axis=1).astype(np.int64)


def reduce_pairs(rb, n, k):
    """the pair batch's answers, [text][member], reduced by the key (score, panel index)"""
    sc = rb.scores()[0].reshape(n, k).astype(np.int64)
    ts, te = (x.reshape(n, k) for x in rb.locations())
    key = np.where(sc >= 0, sc * (k + 1) + np.arange(k)[None, :], np.iinfo(np.int64).max)
    two = np.argpartition(key, 1, axis=1)[:, :2]
    rows = np.arange(n)
    swap = key[rows, two[:, 0]] > key[rows, two[:, 1]]
    b = np.where(swap, two[:, 1], two[:, 0])
    r = np.where(swap, two[:, 0], two[:, 1])
    has1, has2 = sc[rows, b] >= 0, sc[rows, r] >= 0
    out = np.full((n, 6), -1, dtype=np.int64)
    out[has1, 0] = b[has1]; out[has1, 1] = sc[rows, b][has1]; out[has1, 2] = ts[rows, b][has1]; out[has1, 3] = te[rows, b][has1]
    out[has2, 4] = r[has2]; out[has2, 5] = sc[rows, r][has2]
    return out


def timed(ways, rounds):
    """ways: {name: callable -> kernel ms or None}; -> {name: {wall, kernel}} over the rounds, alternating, one warm-up round"""
    wall = {k: [] for k in ways}
    kern = {k: [] for k in ways}
    for rnd in range(rounds + 1):
        for name, fn in ways.items():
            t0 = time.perf_counter()
            ms = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd > 0:
                wall[name].append(dt)
                if ms is not None:
                    kern[name].append(ms)
    return {k: dict(wall_ms=stat(wall[k]), **({"kernel_ms": stat(kern[k])} if kern[k] else {})) for k in ways}


def leg_a(capi, datagen, rounds, n):
    k, m, length, bound = 96, 24, 150, 4
    panel, texts = make_set(n, k, m, length, 0.08, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(k)]
    rb = capi.ResidentBatch(text_batch(texts, datagen))
    rq = capi.ResidentBatch(pair_batch(panel, texts, datagen))

    def panel_way():
        rb.kernel_times()
        assert rb.run_panel(capi.SEARCH_INFIX, members, bound) == capi.QUICKED_OK
        panel_way.out = panel_answers(rb)
        return float(rb.kernel_times()[0][0])

    def pair_way():
        rq.kernel_times()
        assert rq.run_search(capi.SEARCH_INFIX, bound, only_score=True) == capi.QUICKED_OK
        pair_way.out = reduce_pairs(rq, n, k)
        return float(rq.kernel_times()[0][0])

    panel_way()
    pair_way()
    differ = int((panel_way.out != pair_way.out).any(axis=1).sum())
    assert differ == 0, f"leg a: the two routes differ on {differ} texts"
    out = dict(leg="a", texts=n, members=k, member_bases=m, text_bases=length, bound=bound, mode="infix",
               with_best=int((panel_way.out[:, 0] >= 0).sum()), with_runner_up=int((panel_way.out[:, 4] >= 0).sum()),
               ways=timed({"panel": panel_way, "pairs": pair_way}, rounds))
    out["panel_against_pairs"] = verdict(out["ways"]["panel"]["wall_ms"], out["ways"]["pairs"]["wall_ms"])
    rb.close()
    rq.close()
    return out


def leg_b(capi, datagen, rounds, n, count_search):
    k, m, length, bound = 96, 24, 150, 4
    panel, texts = make_set(n, k, m, length, 0.08, 32)
    members = [ACGT[panel[p]].tobytes() for p in range(k)]
    rb = capi.ResidentBatch(text_batch(texts, datagen))
    steps = {}

    def panel_way():
        rb.kernel_times()
        assert rb.run_panel(capi.SEARCH_INFIX, members, bound) == capi.QUICKED_OK
        panel_answers(rb)
        steps["panel"] = int(rb.counters()[0])
        return float(rb.kernel_times()[0][0])

    out = dict(leg="b", texts=n, members=k, member_bases=m, text_bases=length, bound=bound, mode="infix", ways=timed({"panel": panel_way}, rounds))
    rb.close()
    # k_search, both forms, on leg a of tools/search_bench.py
    import search_bench
    leg = dict(search_bench.LEGS["a"])
    if count_search:
        leg["count"] = count_search
    base = datagen.generate(leg["count"], leg["m"], leg["error"], seed=leg["seed"])
    rs = capi.ResidentBatch(search_bench.embed(base, leg["n"], leg["seed"] + 1000, datagen))

    def search_way(form):
        def fn():
            os.environ["QE_SEARCH_FORM"] = form
            capi.reload_env()
            rs.kernel_times()
            assert rs.run_search(capi.SEARCH_INFIX, leg["bound"], only_score=True) == capi.QUICKED_OK
            rs.scores(), rs.locations()
            steps["search_" + form] = int(rs.counters()[0])
            return float(rs.kernel_times()[0][0])
        return fn

    out["ways"].update(timed({"search_workspace": search_way("0"), "search_registers": search_way("1")}, rounds))
    os.environ.pop("QE_SEARCH_FORM", None)
    capi.reload_env()
    rs.close()
    out["block_steps"] = dict(panel=steps["panel"], search_workspace=steps["search_0"], search_registers=steps["search_1"])
    out["ps_per_block_step"] = {w: round(out["ways"][w]["kernel_ms"]["median"] * 1e9 / out["block_steps"][w], 3) for w in out["block_steps"]}
    return out


def leg_c(capi, datagen, rounds, n, k):
    m, length, bound = 24, 150, 4
    panel, texts = make_set(n, k, m, length, 0.08, 33)
    members = [ACGT[panel[p]].tobytes() for p in range(k)]
    rb = capi.ResidentBatch(text_batch(texts, datagen))
    answers = {}

    def way(slices):
        def fn():
            if slices is None:
                os.environ.pop("QE_PANEL_SLICES", None)
            else:
                os.environ["QE_PANEL_SLICES"] = slices
            capi.reload_env()
            rb.kernel_times()
            assert rb.run_panel(capi.SEARCH_INFIX, members, bound) == capi.QUICKED_OK
            answers[slices] = panel_answers(rb)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="c", texts=n, members=k, member_bases=m, text_bases=length, bound=bound, mode="infix",
               ways=timed({"one_slice": way("1"), "host_choice": way(None)}, rounds))
    os.environ.pop("QE_PANEL_SLICES", None)
    capi.reload_env()
    assert (answers["1"] == answers[None]).all()
    out["host_choice_against_one_slice"] = verdict(out["ways"]["host_choice"]["wall_ms"], out["ways"]["one_slice"]["wall_ms"])
    rb.close()
    return out


def leg_d(capi, pcapi, datagen, rounds, count):
    import search_bench
    leg = dict(search_bench.LEGS["a"])
    if count:
        leg["count"] = count
    base = datagen.generate(leg["count"], leg["m"], leg["error"], seed=leg["seed"])
    batch = search_bench.embed(base, leg["n"], leg["seed"] + 1000, datagen)
    rbs = {"this": (capi, capi.ResidentBatch(batch)), "parent": (pcapi, pcapi.ResidentBatch(batch))}
    answers = {}

    def way(name):
        c, rb = rbs[name]

        def fn():
            rb.kernel_times()
            assert rb.run_search(c.SEARCH_INFIX, leg["bound"], only_score=True) == c.QUICKED_OK
            answers[name] = np.stack([rb.scores()[0]] + list(rb.locations()), axis=1)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="d", pairs=leg["count"], pattern=leg["m"], text=leg["n"], bound=leg["bound"], mode="infix",
               ways=timed({"parent": way("parent"), "this": way("this")}, rounds))
    assert (answers["this"] == answers["parent"]).all()
    out["this_against_parent_wall"] = verdict(out["ways"]["this"]["wall_ms"], out["ways"]["parent"]["wall_ms"])
    out["this_against_parent_kernel"] = verdict(out["ways"]["this"]["kernel_ms"], out["ways"]["parent"]["kernel_ms"])
    for _, rb in rbs.values():
        rb.close()
    return out


def row(name, w):
    a = w["wall_ms"]
    k = w.get("kernel_ms")
    return f"| {name} | {a['min']} / {a['median']} / {a['max']} | " + (f"{k['min']} / {k['median']} / {k['max']}" if k else "") + " |"


def markdown(out):
    lines = ["# Panel runs: what was measured", "",
             f"`python tools/search_panel_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*sync call*: host clock around the call and the getters that bring its answers into numpy arrays (for the pair route: the",
             "reduction by the key too).  *kernels*: `quicked_batch_kernel_times` slot 0, the search passes alone.  A way is called ahead",
             "or behind only where the medians differ by more than the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] == "a":
            lines += [f"## a: {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, bound {leg['bound']}", "",
                      f"The two routes agreed on every field of every text ({leg['with_best']} texts with a best member, {leg['with_runner_up']} with a runner-up).", "",
                      "| route | sync call | kernels |", "|---|---|---|", row("panel run", leg["ways"]["panel"]),
                      row(f"{leg['texts'] * leg['members']}-pair batch through run_search + numpy reduction", leg["ways"]["pairs"]), "",
                      f"The panel run is **{leg['panel_against_pairs']}** (sync call).  The pair batch was resident before the timing: its upload and its {leg['members']} copies of every text in HBM are not in these figures.", ""]
        elif leg["leg"] == "b":
            lines += [f"## b: the panel run alone, {leg['texts']} texts x {leg['members']} members", "", "| run | sync call | kernels | block steps | ps per block step |", "|---|---|---|---|---|"]
            for w, label in (("panel", "panel run"), ("search_workspace", "k_search, workspace form (search leg a)"), ("search_registers", "k_search, register form (search leg a)")):
                lines.append(row(label, leg["ways"][w]) + f" {leg['block_steps'][w]} | {leg['ps_per_block_step'][w]} |")
            lines += [""]
        elif leg["leg"] == "c":
            lines += [f"## c: {leg['texts']} texts x {leg['members']} members: slices", "", "| slices | sync call | kernels |", "|---|---|---|",
                      row("QE_PANEL_SLICES=1", leg["ways"]["one_slice"]), row("the host's choice", leg["ways"]["host_choice"]), "",
                      f"The host's choice is **{leg['host_choice_against_one_slice']}** of one slice (sync call).", ""]
        elif leg["leg"] == "d":
            lines += [f"## d: the unflagged best search, parent commit against this one ({leg['pairs']} pairs, {leg['pattern']} in {leg['text']}, bound {leg['bound']}, INFIX)", "",
                      "| library | sync call | kernels |", "|---|---|---|", row("parent", leg["ways"]["parent"]), row("this", leg["ways"]["this"]), "",
                      f"This commit is **{leg['this_against_parent_wall']}** with its parent on the sync call and **{leg['this_against_parent_kernel']}** on the kernels.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no leg d)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", nargs="*", default=["a", "b", "c", "d"])
    ap.add_argument("--scale", type=float, default=1.0, help="scale the legs' text counts (smoke runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.rounds >= 7 or args.scale < 1, "medians of at least 7 rounds"
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    s = args.scale
    legs = []
    for leg in args.legs:
        if leg == "a":
            legs.append(leg_a(capi, datagen, args.rounds, max(64, int(100_000 * s))))
        elif leg == "b":
            legs.append(leg_b(capi, datagen, args.rounds, max(64, int(1_000_000 * s)), 0 if s >= 1 else max(64, int(1_000_000 * s))))
        elif leg == "c":
            legs.append(leg_c(capi, datagen, args.rounds, max(64, int(2000 * s)), 4096))
        elif leg == "d" and args.parent:
            pcapi = load_package(os.path.abspath(args.parent), "parent_quicked_amd")
            assert not hasattr(pcapi, "PANEL_MATRIX"), "--parent must be a tree without panel runs"
            legs.append(leg_d(capi, pcapi, datagen, args.rounds, 0 if s >= 1 else max(64, int(1_000_000 * s))))
        print(json.dumps(legs[-1]) if legs else "{}", flush=True)
    out = dict(unit="ms", rounds=args.rounds, scale=s, session=time.strftime("%Y-%m-%d"), legs=legs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
