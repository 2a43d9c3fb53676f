"""The 3' tails of the panel search on the GPU (QUICKED_PANEL_TAILS through capi.ResidentBatch.run_panel_all and panel_tails()):
the member cut off by every text's end.  Expected tails never come from the library: they are tests/panel_tails_lib.py's -- the
full matrix and the rule in Python -- recorded in tests/golden/panel_tails_cases.json (a sample of which
tests/test_panel_tails_cpu.py recomputes) or computed live for the sets made here.  Every flagged run is held against the same run
without the bit: occurrences, counts, scores, statuses, counter [0] and -- with QUICKED_PANEL_CIGARS -- the strings are
unchanged."""
import importlib.util
import os

import numpy as np
import pytest

import panel_tails_lib as T
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFIX, CG, TL = capi.SEARCH_INFIX, capi.PANEL_CIGARS, capi.PANEL_TAILS
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "4096"]
WIRES = [None, capi.WIRE_2BIT, capi.WIRE_PLANES3]
OCC_FIELDS = ("pattern", "text_start", "text_end", "score")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_tails_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


def _pool(seqs):
    pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    return pool, off, ln


def batch_of(texts, wire=None):
    pp, po, pl = _pool([b""] * len(texts))
    tp, to, tl = _pool(texts)
    return capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl), wire=wire)


def env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def wire_holds(texts, wire):
    """can the wire format carry these texts as the ASCII batch means them?  two bits: A C G T only; three planes: every other
    byte arrives as N, so only N may stand beside the bases"""
    ok = set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN")
    return wire is None or all(set(t) <= ok for t in texts)


def records(rb):
    """-> (found, off, [(pattern, text_start, text_end, score)], scores, statuses, counter [0])"""
    found, _ = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    rows = np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64).tolist() if len(hits) else []
    sc, st = rb.scores()
    return found.tolist(), off.tolist(), [tuple(r) for r in rows], sc.tolist(), st.tolist(), int(rb.counters()[0])


def tails_of(rb):
    a = rb.panel_tails()
    return [tuple(int(a[f][i]) for f in T.TAIL_FIELDS) for i in range(len(a))]


def flagged_and_plain(rb, mode, panel, bounds, cap):
    """the run without the bit, then with it: -> the tails; everything the first leaves is left unchanged, counter [0] and the
    strings of a QUICKED_PANEL_CIGARS run included, and the tails exist after the second only"""
    arg = np.asarray(bounds, dtype=np.int32)
    assert rb.run_panel_all(mode, panel, arg, max_hits=cap) == capi.QUICKED_OK
    plain = records(rb)
    plain_s = rb.panel_hit_cigars() if mode & CG else None
    with pytest.raises(capi.QuickedException):
        rb.panel_tails()
    assert rb.counters()[2] == 0
    assert rb.run_panel_all(mode | TL, panel, arg, max_hits=cap) == capi.QUICKED_OK
    assert records(rb) == plain
    if mode & CG:
        assert rb.panel_hit_cigars() == plain_s
    else:
        with pytest.raises(capi.QuickedException):
            rb.panel_hit_cigars()
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix):
        with pytest.raises(capi.QuickedException):
            getter()
    return tails_of(rb)


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("wire", WIRES)
def test_the_sets(sets, wire, nslices, monkeypatch):
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    ran = 0
    for g in sets["named"] + sets["random"]:
        if not wire_holds(g["texts"], wire):
            continue
        rb = batch_of(g["texts"], wire)
        for flag in FLAGS:
            for mo in G.OVERLAPS:
                assert rb.configure_panel_tails(mo) == capi.QUICKED_OK
                for cap, cg in ((1, 0), (64, 0), (64, CG)):
                    got = flagged_and_plain(rb, INFIX | flag | cg, g["panel"], g["bounds"], cap)
                    want = g["tails"][(flag, mo)]
                    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
                    assert not bad, (g["name"], flag, mo, cap, cg, bad[:5])
                    rows = int(rb.counters()[2])
                    most = sum(len(q) - 1 for q in g["panel"]) * sum(len(t) > 0 for t in g["texts"])
                    assert 0 <= rows <= most and (rows > 0 or most == 0)
                    ran += 1
        rb.close()
    assert ran >= 36


def test_a_batch_without_a_full_occurrence_still_has_its_tails():
    """k_panel_hits_count's total is zero and the run ends early; the tails are there all the same"""
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    rng = np.random.default_rng(3)
    texts = [G.rand_seq(rng, 60 + i, "CT") + adapter[:5 + i % 20] for i in range(200)] + [G.rand_seq(rng, 80, "CT"), b""]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | TL, [adapter], 2, max_hits=4) == capi.QUICKED_OK
    found, stored = rb.panel_hit_counts()
    assert int(found.sum()) == 0 and int(stored.sum()) == 0 and len(rb.panel_hits()[1]) == 0
    got = tails_of(rb)
    assert got == T.all_tails(texts, [adapter], [2], 0, 3)
    assert all(t[0] == 0 and t[1] >= 5 for t in got[:200]) and got[200] == got[201] == T.NONE
    rb.close()


def test_live_random_set():
    """about 2 000 texts of at most 200 bases against 8 members, made now: at least a third of the texts have a tail and at least a
    third have none, so a run cannot pass by reporting nothing -- or everything"""
    rng = np.random.default_rng(20261020)
    panel = [G.rand_seq(rng, int(m)) for m in rng.integers(18, 41, 8)]
    bounds = [int(b) for b in rng.integers(0, 5, 8)]
    texts = []
    for i in range(2000):
        n = int(rng.integers(1, 201))
        if i % 2:
            p = int(rng.integers(0, 8))
            m = len(panel[p])
            r = int(rng.integers(5, m))
            tail = G.mutate(rng, panel[p][:r], int(rng.integers(0, (r * min(bounds[p], m)) // m + 1)))
            texts.append(G.fit(rng, tail, max(n, 8)))
        else:
            texts.append(G.rand_seq(rng, n))
    want = T.all_tails(texts, panel, bounds, 0, 3)
    have = sum(t[0] >= 0 for t in want)
    assert 3 * have >= len(want) and 3 * (len(want) - have) >= len(want), have
    rb = batch_of(texts)
    got = flagged_and_plain(rb, INFIX, panel, bounds, 16)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, bad[:5]
    rb.close()


def test_the_getter_refuses_after_a_run_without_the_bit_and_the_bit_is_refused_elsewhere():
    texts = [b"CTCTCTCTAGATCGG", b"CTCTCTCT"]
    panel = [b"AGATCGGAAGAGC"]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | TL, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert tails_of(rb) == [(0, 7, 8, 0), T.NONE]
    c = rb.counters().copy()
    # refused with nothing launched: results, tails and counters stay
    assert rb.run_panel_all(capi.SEARCH_PREFIX | TL, panel, 1, max_hits=4) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX | TL, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | TL, panel, 1, max_hits=4, window=64) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | TL | 1024, panel, 1, max_hits=4) == capi.QUICKED_ERROR
    for bad in (0, -1, capi.PANEL_MAX_LEN + 1):
        assert rb.configure_panel_tails(bad) == capi.QUICKED_ERROR
    assert tails_of(rb) == [(0, 7, 8, 0), T.NONE] and (rb.counters() == c).all()
    # min_overlap holds for the runs to come
    assert rb.configure_panel_tails(8) == capi.QUICKED_OK
    assert rb.run_panel_all(INFIX | TL, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert tails_of(rb) == [T.NONE, T.NONE]
    assert rb.configure_panel_tails(3) == capi.QUICKED_OK
    assert rb.run_panel_all(INFIX | TL, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert tails_of(rb) == [(0, 7, 8, 0), T.NONE]
    # a run without the bit after a flagged run: the getter refuses
    assert rb.run_panel_all(INFIX, panel, 1, max_hits=4) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.panel_tails()
    assert rb.counters()[2] == 0
    rb.close()
