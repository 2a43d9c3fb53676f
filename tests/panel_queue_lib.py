"""What the tests of the queued panel runs (quicked_batch_configure_panel_queue) share: the four recorded panel sets as one list of
groups, and what a run of each kind must report on a group BY THE DEFINITIONS -- tests/panel_lib.py (the best member),
tests/panel_hits_lib.py (every occurrence), tests/panel_tails_lib.py and tests/panel_heads_lib.py --, taken from the record where
the fixture holds it and computed by the same functions where it does not.  The overflow rule of a queued all-occurrences run is
restated here once (capped_run).  Nothing in here calls the library."""
import importlib.util
import os

import numpy as np

import panel_heads_lib as H
import panel_hits_lib as PH
import panel_lib as P
import panel_tails_lib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = 1, 2
FLAGS = (0, 16, 32)
TAILS, HEADS = T.TAILS, H.HEADS
FIXTURES = ("search_panel", "panel_hits", "panel_tails", "panel_heads")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GROUPS = {}


def groups(fixture, name):
    """the `named` or `random` set of one fixture, loaded through its make_*_cases.load() -> [group]: name, texts, panel, bounds
    and whatever the fixture records.  Texts of thousands of bases (the windowed run's ground) are left out"""
    key = (fixture, name)
    if key not in _GROUPS:
        s = _load("make_%s_cases" % fixture).load()[name]
        gs = [dict(s, name=name)] if isinstance(s, dict) else [dict(g) for g in s]
        _GROUPS[key] = [dict(g, fixture=fixture) for g in gs if max(len(t) for t in g["texts"]) <= 1000]
    return _GROUPS[key]


_DEFS = {}


def _cached(g, what, make):
    key = (g["fixture"], g["name"], tuple(g["bounds"])) + what
    if key not in _DEFS:
        _DEFS[key] = make()
    return _DEFS[key]


def hits(g, mode, flag):
    """every text's uncapped occurrence list [(pattern, text_start, text_end, score)] under the members' own bounds"""
    if "hits" in g:
        return g["hits"][(mode, flag, "own")]
    return _cached(g, ("hits", mode, flag), lambda: PH.all_hits(g["texts"], g["panel"], g["bounds"], mode, flag))


def best(g, mode, flag):
    """every text's quicked_panel_hit_t as six ints: panel_lib's over the recorded matrix, else consequence 1 of the header --
    the smallest key among the text's occurrences -- over panel_hits_lib's lists"""
    if "matrix" in g:
        return _cached(g, ("best", mode, flag), lambda: P.expected(g["texts"], g["panel"], g["bounds"], mode, flag, *g["matrix"][(mode, flag)])[0].tolist())
    return [list(PH.best_two(h)) for h in hits(g, mode, flag)]


def tails(g, flag, min_overlap):
    if "tails" in g:
        return g["tails"][(flag, min_overlap)]
    return _cached(g, ("tails", flag, min_overlap), lambda: T.all_tails(g["texts"], g["panel"], g["bounds"], flag, min_overlap))


def heads(g, flag, min_overlap):
    if "heads" in g:
        return g["heads"][(flag, min_overlap)]
    return _cached(g, ("heads", flag, min_overlap), lambda: H.all_heads(g["texts"], g["panel"], g["bounds"], flag, min_overlap))


def capped_run(lists, max_hits, max_total):
    """the uncapped lists -> (found [n], hit_off' [n + 1], the records in order, scores [n], W): the cap per text, then the room
    per run -- the first max_total records of the array in the order of the pairs"""
    found = [len(h) for h in lists]
    stored = [h[:max_hits] for h in lists]
    off = np.concatenate([[0], np.cumsum([len(h) for h in stored])]).astype(np.int64)
    W = int(off[-1])
    recs = [o for h in stored for o in h][:max_total]
    scores = [min(o[3] for o in h) if h else -1 for h in lists]
    return found, np.minimum(off, max_total).tolist(), [tuple(int(v) for v in o) for o in recs], scores, W


def cases_file(path, gs, overlaps=(1, 3)):
    """the input of tests/native/panel_queue_host.cpp: the number of groups and per group "K n", K x {member bound}, n x text
    ("." = empty), then per flag of FLAGS: per base mode PREFIX, INFIX n x {found, found x {pattern text_start text_end
    score}} uncapped; per min_overlap n x {the tail's four fields} and n x {the head's four fields}; the overlaps on the last line"""
    lines = ["%d %d" % (len(gs), len(overlaps))]
    for g in gs:
        lines.append("%d %d" % (len(g["panel"]), len(g["texts"])))
        lines += ["%s %d" % (q.decode(), b) for q, b in zip(g["panel"], g["bounds"])]
        lines += [t.decode() or "." for t in g["texts"]]
        for flag in FLAGS:
            for mode in (PREFIX, INFIX):
                for h in hits(g, mode, flag):
                    lines.append(" ".join([str(len(h))] + [str(int(v)) for o in h for v in o]))
            for mo in overlaps:
                lines += [" ".join(str(int(v)) for v in t) for t in tails(g, flag, mo)]
                lines += [" ".join(str(int(v)) for v in t) for t in heads(g, flag, mo)]
    lines.append(" ".join(str(mo) for mo in overlaps))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
