#!/usr/bin/env python3
"""Queued panel runs (quicked_batch_configure_panel_queue): a stream of batches against one panel, queued against sync; whether
the sync runs moved; what the room of a queued all-occurrences run costs.

    python tools/panel_queue_bench.py [--parent <built tree of the parent commit>] [--rounds 7] --out profiles/panel_queue.json

The procedure of tools/panel_heads_bench.py: one process, medians of `rounds` rounds after one warm-up round, with min and max;
the ways of a leg alternate round by round, and every way brings its answers into numpy arrays inside the timed stretch.
Everything uses the README's panel workload -- 100 000 texts of 150 bases x 96 members of 24 bases, INFIX, bound 4, every text
holding one member with 8 % of its bases substituted -- at max_hits 16.
    stream  32 fresh batches of that workload, for run_panel, run_panel_all and run_panel_all | TAILS | HEADS:
            a  (--parent) the parent commit's route: one batch object, reload + sync run + getters per batch;
            b  the same route on this commit;
            c  queued: four batch objects in rotation, an uploader thread reloading ahead, the main thread queueing, a third
               thread fetching and reading the getters behind, at most two runs queued and not fetched (bench.py's end-to-end
               leg).  Its answers are asserted equal to b's on every batch before anything is timed.
            ms per batch, and quicked_batch_kernel_times slot 0 per batch beside it.
    sync    (--parent) the three runs with sync != 0 on one resident batch, the parent's library and this one alternating.
    room    one queued run_panel_all with max_total = W, 4 W and texts x max_hits: the kernels of the run.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import search_panel_bench as SPB      # noqa: E402
import panel_heads_bench as PHB       # noqa: E402

ACGT = SPB.ACGT
K, M, LENGTH, BOUND, MAX_HITS = 96, 24, 150, 4, 16
KINDS = ("panel", "panel_all", "panel_all_tails_heads")
SLOTS, INFLIGHT = 4, 2


def run_kind(c, rb, kind, members, sync):
    if kind == "panel":
        return rb.run_panel(c.SEARCH_INFIX, members, BOUND, sync=sync)
    bits = (2048 | 8192) if kind == "panel_all_tails_heads" else 0
    return rb.run_panel_all(c.SEARCH_INFIX | bits, members, BOUND, max_hits=MAX_HITS, sync=sync)


def answers(rb, kind):
    if kind == "panel":
        return (SPB.panel_answers(rb),)
    out = PHB.records(rb)
    return out + ((PHB.tails(rb), PHB.heads(rb)) if kind == "panel_all_tails_heads" else ())


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def sync_stream(c, rb, kind, members, batches):
    """reload + sync run + getters per batch on one batch object -> (answers per batch, kernel ms of the stream)"""
    rb.kernel_times()
    out = []
    for tb in batches:
        assert rb.reload(tb) >= 0
        assert run_kind(c, rb, kind, members, True) == c.QUICKED_OK
        out.append(answers(rb, kind))
    ms, launches = rb.kernel_times()
    sync_stream.launches = int(launches[0])
    return out, float(ms[0])


def queued_stream(c, rbs, kind, members, batches):
    """bench.py's end-to-end leg for panel runs -> (answers per batch, kernel ms of the stream)"""
    nb = len(batches)
    uploaded, queued, on_host, fetched = ([threading.Event() for _ in range(nb)] for _ in range(4))
    out, err = [None] * nb, []

    def fail(e):
        err.append(e)
        for ev in uploaded + queued + on_host + fetched:
            ev.set()

    def uploader():
        try:
            for k in range(nb):
                if k >= SLOTS:
                    fetched[k - SLOTS].wait()
                if err:
                    return
                assert rbs[k % SLOTS].reload(batches[k]) >= 0
                uploaded[k].set()
        except Exception as e:      # noqa: BLE001
            fail(e)

    def fetcher():
        try:
            for k in range(nb):
                queued[k].wait()
                if err:
                    return
                rb = rbs[k % SLOTS]
                assert rb.fetch() == c.QUICKED_OK
                on_host[k].set()
                out[k] = answers(rb, kind)
                fetched[k].set()
        except Exception as e:      # noqa: BLE001
            fail(e)

    rbs[0].kernel_times()
    ths = [threading.Thread(target=uploader), threading.Thread(target=fetcher)]
    for th in ths:
        th.start()
    try:
        for k in range(nb):
            uploaded[k].wait()
            if k >= INFLIGHT:
                on_host[k - INFLIGHT].wait()
            if err:
                break
            assert run_kind(c, rbs[k % SLOTS], kind, members, False) == c.QUICKED_OK
            queued[k].set()
    except Exception as e:      # noqa: BLE001
        fail(e)
    for th in ths:
        th.join()
    if err:
        raise err[0]
    ms, launches = rbs[0].kernel_times()                  # (the queueing thread's launches: every timed kernel of every run)
    queued_stream.launches = int(launches[0])
    return out, float(ms[0])


def leg_stream(capi, pcapi, datagen, rounds, n, nbatches):
    panel = SPB.make_set(64, K, M, LENGTH, 0.08, 31)[0]
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    batches = []
    for k in range(nbatches):
        rng = np.random.default_rng(1000 + k)
        texts = rng.integers(0, 4, (n, LENGTH), dtype=np.uint8)
        which, at = rng.integers(0, K, n), rng.integers(0, LENGTH - M + 1, n)
        planted = panel[which]
        planted = np.where(rng.random((n, M)) < 0.08, (planted + rng.integers(1, 4, (n, M), dtype=np.uint8)) % 4, planted).astype(np.uint8)
        texts[np.arange(n)[:, None], at[:, None] + np.arange(M)[None, :]] = planted
        third = np.arange(n) % 3 == 0                       # (heads and tails to find: a third of the texts begin inside a member)
        texts[third, :12] = panel[which[third], M - 12:]
        batches.append(SPB.text_batch(texts, datagen))
    rb_b = capi.ResidentBatch(batches[0])
    rb_a = pcapi.ResidentBatch(batches[0]) if pcapi else None
    rbs = [capi.ResidentBatch(batches[0]) for _ in range(SLOTS)]
    for rb in rbs:
        assert rb.configure_panel_queue(n * MAX_HITS) == capi.QUICKED_OK
    out = dict(leg="stream", texts=n, batches=nbatches, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS,
               slots=SLOTS, inflight=INFLIGHT, max_total=n * MAX_HITS, kinds={})
    for kind in KINDS:
        # quicked_batch_kernel_times collects the timed launches of the CALLING thread's context, whichever batch objects they
        # served: the queueing thread's launch count over the rotation is recorded beside the sync route's on one object
        want, _ = sync_stream(capi, rb_b, kind, members, batches)
        launches_b = sync_stream.launches
        got, _ = queued_stream(capi, rbs, kind, members, batches)
        launches_c = queued_stream.launches
        for k in range(nbatches):
            assert same(got[k], want[k]), f"{kind}: the queued stream differs from the sync route on batch {k}"
        if rb_a:
            old, _ = sync_stream(pcapi, rb_a, kind, members, batches)
            assert all(same(o, w) for o, w in zip(old, want)), f"{kind}: this commit's sync route differs from the parent's"
        del want, got
        ways = {}
        if rb_a:
            ways["a"] = lambda kind=kind: sync_stream(pcapi, rb_a, kind, members, batches)[1]
        ways["b"] = lambda kind=kind: sync_stream(capi, rb_b, kind, members, batches)[1]
        ways["c"] = lambda kind=kind: queued_stream(capi, rbs, kind, members, batches)[1]
        t = SPB.timed(ways, rounds)
        per = {w: {what: SPB.stat([x / nbatches for x in t[w][what]["samples"]]) for what in ("wall_ms", "kernel_ms")} for w in t}
        base = "a" if rb_a else "b"
        out["kinds"][kind] = dict(ways=per, baseline=base, timed_launches_per_batch=dict(b=launches_b / nbatches, c=launches_c / nbatches), queued_against_baseline=SPB.verdict(per["c"]["wall_ms"], per[base]["wall_ms"]),
                                  queued_over_baseline=round(per["c"]["wall_ms"]["median"] / per[base]["wall_ms"]["median"], 4),
                                  **({"b_against_a": SPB.verdict(per["b"]["wall_ms"], per["a"]["wall_ms"])} if rb_a else {}))
    for rb in rbs + [rb_b] + ([rb_a] if rb_a else []):
        rb.close()
    return out


def leg_sync(capi, pcapi, datagen, rounds, n):
    panel, texts, _, _ = PHB.make_set(n, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    tb = SPB.text_batch(texts, datagen)
    rbs = {"parent": (pcapi, pcapi.ResidentBatch(tb)), "this": (capi, capi.ResidentBatch(tb))}
    got = {}

    def way(kind, name):
        c, rb = rbs[name]

        def fn():
            rb.kernel_times()
            assert run_kind(c, rb, kind, members, True) == c.QUICKED_OK
            got[kind, name] = answers(rb, kind)
            return float(rb.kernel_times()[0][0])
        return fn

    out = dict(leg="sync", texts=n, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, ways={})
    for kind in KINDS:
        out["ways"].update(SPB.timed({f"{kind}_parent": way(kind, "parent"), f"{kind}_this": way(kind, "this")}, rounds))
        assert same(got[kind, "this"], got[kind, "parent"]), kind
        for what in ("wall_ms", "kernel_ms"):
            out[f"{kind}_this_against_parent_{what}"] = SPB.verdict(out["ways"][kind + "_this"][what], out["ways"][kind + "_parent"][what])
    for _, rb in rbs.values():
        rb.close()
    return out


def leg_room(capi, datagen, rounds, n):
    panel, texts, _, _ = PHB.make_set(n, 31)
    members = [ACGT[panel[p]].tobytes() for p in range(K)]
    rb = capi.ResidentBatch(SPB.text_batch(texts, datagen))
    assert rb.run_panel_all(capi.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
    want = PHB.records(rb)
    W = int(want[1][-1])
    rooms = {"W": W, "4W": min(4 * W, n * MAX_HITS), "texts_x_max_hits": n * MAX_HITS}

    def way(room):
        def fn():
            assert rb.configure_panel_queue(room) == capi.QUICKED_OK
            rb.kernel_times()
            assert rb.run_panel_all(capi.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS, sync=False) == capi.QUICKED_OK
            assert rb.fetch() == capi.QUICKED_OK
            assert rb.panel_queue_wanted() == W and same(PHB.records(rb), want)
            return float(rb.kernel_times()[0][0])
        return fn

    def sync_way():
        rb.kernel_times()
        assert rb.run_panel_all(capi.SEARCH_INFIX, members, BOUND, max_hits=MAX_HITS) == capi.QUICKED_OK
        PHB.records(rb)
        return float(rb.kernel_times()[0][0])

    ways = {name: way(room) for name, room in rooms.items()}
    ways["sync"] = sync_way
    out = dict(leg="room", texts=n, members=K, member_bases=M, text_bases=LENGTH, bound=BOUND, max_hits=MAX_HITS, W=W, rooms=rooms, ways=SPB.timed(ways, rounds))
    for name in rooms:
        out[f"{name}_against_sync_kernel_ms"] = SPB.verdict(out["ways"][name]["kernel_ms"], out["ways"]["sync"]["kernel_ms"])
    out["widest_against_W_kernel_ms"] = SPB.verdict(out["ways"]["texts_x_max_hits"]["kernel_ms"], out["ways"]["W"]["kernel_ms"])
    rb.close()
    return out


def markdown(out):
    row = SPB.row
    lines = ["# Queued panel runs (quicked_batch_configure_panel_queue): what was measured", "",
             f"`python tools/panel_queue_bench.py --parent <built tree of the parent commit> --rounds {out['rounds']}` on one MI355X, one process, one",
             "session" + (f" ({out['session']})" if out.get("session") else "") + (f", text counts scaled by {out['scale']}" if out["scale"] != 1 else "") +
             ".  ms, min / median / max over the rounds after one warm-up round; the ways of a leg alternate round by round.",
             "*kernels*: `quicked_batch_kernel_times` slot 0.  A way is called ahead or behind only where the medians differ by more than",
             "the larger of the two spreads (DESIGN.md 4.9), else level.", ""]
    for leg in out["legs"]:
        if leg["leg"] == "stream":
            lines += [f"## 1. Stream: {leg['batches']} fresh batches of {leg['texts']} texts of {leg['text_bases']} x {leg['members']} members of {leg['member_bases']}, INFIX, bound {leg['bound']}, max_hits {leg['max_hits']}", "",
                      "ms per batch.  (a) the parent commit's library: one batch object, reload + sync run + getters per batch; (b) the same route on this",
                      f"commit; (c) queued: {leg['slots']} batch objects in rotation, an uploader thread reloading ahead, a fetching thread behind, at most {leg['inflight']} runs",
                      f"queued and not fetched, max_total = {leg['max_total']}.  (c)'s answers equal (b)'s on every batch (asserted before timing).", ""]
            for kind, r in leg["kinds"].items():
                lines += [f"### {kind}", "", "| route | per batch | kernels per batch |", "|---|---|---|"]
                lines += [row({"a": "(a) parent, sync", "b": "(b) this commit, sync", "c": "(c) this commit, queued"}[w], r["ways"][w]) for w in r["ways"]]
                lines += ["", f"Timed launches per batch: {r['timed_launches_per_batch']['b']:g} on route (b), {r['timed_launches_per_batch']['c']:g} on route (c) (read from the queueing thread).",
                          f"(c) is **{r['queued_against_baseline']}** ({r['queued_over_baseline']} x) against the baseline ({r['baseline']})" +
                          (f"; (b) is **{r['b_against_a']}** with (a)." if "b_against_a" in r else "."), ""]
        elif leg["leg"] == "sync":
            lines += [f"## 2. Sync runs unchanged: parent commit against this one ({leg['texts']} texts, one resident batch)", "",
                      "| run, library | sync call | kernels |", "|---|---|---|"]
            for kind in KINDS:
                for lib in ("parent", "this"):
                    lines.append(row(f"{kind}, {lib}", leg["ways"][f"{kind}_{lib}"]))
            lines += [""] + [f"{kind}: this commit is **{leg[kind + '_this_against_parent_wall_ms']}** with its parent on the sync call and **{leg[kind + '_this_against_parent_kernel_ms']}** on the kernels."
                             for kind in KINDS] + [""]
        elif leg["leg"] == "room":
            lines += [f"## 3. The cost of room: one queued run_panel_all, W = {leg['W']} stored occurrences of {leg['texts']} texts", "",
                      "| max_total | queue + fetch + getters | kernels |", "|---|---|---|"]
            lines += [row(f"{name} = {room}", leg["ways"][name]) for name, room in leg["rooms"].items()]
            lines += [row("(the sync run)", leg["ways"]["sync"]), "",
                      f"On the kernels the widest room is **{leg['widest_against_W_kernel_ms']}** with max_total = W; against the sync run: " +
                      ", ".join(f"{name} **{leg[name + '_against_sync_kernel_ms']}**" for name in leg["rooms"]) + ".", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checked-out and built tree of the parent commit (omit: no route a, no leg sync)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", nargs="*", default=["stream", "sync", "room"])
    ap.add_argument("--scale", type=float, default=1.0, help="scale the legs' text counts (smoke runs)")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.rounds >= 7 or args.scale < 1, "medians of at least 7 rounds"
    for name in ("QE_SEARCH_FORM", "QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QUICKED_HIP_LIB"):
        os.environ.pop(name, None)
    from quicked_amd import capi, datagen
    pcapi = None
    if args.parent:
        pcapi = SPB.load_package(os.path.abspath(args.parent), "parent_quicked_amd")
        assert not hasattr(pcapi.ResidentBatch, "configure_panel_queue"), "--parent must be a tree without the queued panel runs"
    n = max(64, int(100_000 * args.scale))
    legs = []
    for leg in args.legs:
        if leg == "stream":
            legs.append(leg_stream(capi, pcapi, datagen, args.rounds, n, args.batches))
        elif leg == "sync" and pcapi:
            legs.append(leg_sync(capi, pcapi, datagen, args.rounds, n))
        elif leg == "room":
            legs.append(leg_room(capi, datagen, args.rounds, n))
        else:
            continue
        print(json.dumps(legs[-1]), flush=True)
    out = dict(unit="ms", rounds=args.rounds, scale=args.scale, session=time.strftime("%Y-%m-%d"), legs=legs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{" + ",\n ".join(json.dumps(k) + ": " + json.dumps(v) for k, v in out.items()).replace('{"leg"', '\n  {"leg"') + "}\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
            f.write(markdown(out))


if __name__ == "__main__":
    main()
