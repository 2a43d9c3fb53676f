"""The 5' heads of the panel search on the GPU (QUICKED_PANEL_HEADS through capi.ResidentBatch.run_panel_all and panel_heads()):
the member cut off by every text's start.  Expected heads never come from the library: they are tests/panel_heads_lib.py's -- the
tails of the reversed texts against the reversed members, from the full matrix in Python -- recorded in
tests/golden/panel_heads_cases.json (a sample of which tests/test_panel_heads_cpu.py recomputes) or computed live for the sets made
here.  Every flagged run is held against the same run without the bit: occurrences, counts, scores, statuses, counters [0] .. [3],
-- with QUICKED_PANEL_CIGARS -- the strings and -- with QUICKED_PANEL_TAILS -- the tails are unchanged."""
import importlib.util
import os

import numpy as np
import pytest

import panel_heads_lib as H
import panel_tails_lib as T
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFIX, PREFIX, CG, TL, HD = capi.SEARCH_INFIX, capi.SEARCH_PREFIX, capi.PANEL_CIGARS, capi.PANEL_TAILS, capi.PANEL_HEADS
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "4096"]
WIRES = [None, capi.WIRE_2BIT, capi.WIRE_PLANES3]
OCC_FIELDS = ("pattern", "text_start", "text_end", "score")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_heads_cases")


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
    """-> (found, off, [(pattern, text_start, text_end, score)], scores, statuses, counters [0] .. [3])"""
    found, _ = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    rows = np.stack([hits[f] for f in OCC_FIELDS], axis=1).astype(np.int64).tolist() if len(hits) else []
    sc, st = rb.scores()
    return found.tolist(), off.tolist(), [tuple(r) for r in rows], sc.tolist(), st.tolist(), [int(c) for c in rb.counters()[:4]]


def heads_of(rb):
    a = rb.panel_heads()
    return [tuple(int(a[f][i]) for f in H.HEAD_FIELDS) for i in range(len(a))]


def tails_of(rb):
    a = rb.panel_tails()
    return [tuple(int(a[f][i]) for f in T.TAIL_FIELDS) for i in range(len(a))]


def flagged_and_plain(rb, mode, panel, bounds, cap):
    """the run without the bit, then with it: -> the heads; everything the first leaves is left unchanged, counters [0] .. [3],
    the strings of a QUICKED_PANEL_CIGARS run and the tails of a QUICKED_PANEL_TAILS run included, and the heads and counters
    [6] and [7] exist after the second only"""
    arg = np.asarray(bounds, dtype=np.int32)
    assert rb.run_panel_all(mode, panel, arg, max_hits=cap) == capi.QUICKED_OK
    plain = records(rb)
    plain_s = rb.panel_hit_cigars() if mode & CG else None
    plain_t = tails_of(rb) if mode & TL else None
    with pytest.raises(capi.QuickedException):
        rb.panel_heads()
    assert rb.counters()[6] == 0 and rb.counters()[7] == 0
    assert rb.run_panel_all(mode | HD, panel, arg, max_hits=cap) == capi.QUICKED_OK
    assert records(rb) == plain
    if mode & CG:
        assert rb.panel_hit_cigars() == plain_s
    else:
        with pytest.raises(capi.QuickedException):
            rb.panel_hit_cigars()
    if mode & TL:
        assert tails_of(rb) == plain_t
    else:
        with pytest.raises(capi.QuickedException):
            rb.panel_tails()
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix):
        with pytest.raises(capi.QuickedException):
            getter()
    return heads_of(rb)


def step_bounds(texts, panel, bounds):
    """-> (the most block steps the short sweep can take, the most row steps of its walk)"""
    steps = sum((len(q) + 63) // 64 * min(len(t), H.reach(q, b)) for t in texts for q, b in zip(panel, bounds))
    rows = sum(len(q) - 1 for q in panel) * sum(len(t) > 0 for t in texts)
    return steps, rows


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("wire", WIRES)
def test_the_sets(sets, wire, nslices, monkeypatch):
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    ran = 0
    for g in sets["named"] + sets["random"]:
        if not wire_holds(g["texts"], wire):
            continue
        rb = batch_of(g["texts"], wire)
        most_steps, most_rows = step_bounds(g["texts"], g["panel"], g["bounds"])
        for flag in FLAGS:
            for mo in G.OVERLAPS:
                assert rb.configure_panel_heads(mo) == capi.QUICKED_OK
                for base, cap, bits in ((INFIX, 1, 0), (INFIX, 64, 0), (INFIX, 64, CG), (INFIX, 64, TL), (INFIX, 64, CG | TL), (PREFIX, 64, 0)):
                    got = flagged_and_plain(rb, base | flag | bits, g["panel"], g["bounds"], cap)
                    want = g["heads"][(flag, mo)]
                    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
                    assert not bad, (g["name"], flag, mo, base, cap, bits, bad[:5])
                    steps, rows = int(rb.counters()[6]), int(rb.counters()[7])
                    assert 0 < steps <= most_steps, (g["name"], steps, most_steps)
                    assert 0 <= rows <= most_rows and (rows > 0 or most_rows == 0)
                    ran += 1
        rb.close()
    assert ran >= 72


def test_a_batch_without_a_full_occurrence_still_has_its_heads():
    """k_panel_hits_count's total is zero and the run ends early; the heads are there all the same"""
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    rng = np.random.default_rng(3)
    texts = [adapter[-(5 + i % 20):] + G.rand_seq(rng, 60 + i, "CT") for i in range(200)] + [G.rand_seq(rng, 80, "CT"), b""]
    want = H.all_heads(texts, [adapter], [2], 0, 3)
    assert all(t[0] == 0 and t[1] >= 5 for t in want[:200]) and want[200] == want[201] == H.NONE
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | HD, [adapter], 2, max_hits=4) == capi.QUICKED_OK
    found, stored = rb.panel_hit_counts()
    assert int(found.sum()) == 0 and int(stored.sum()) == 0 and len(rb.panel_hits()[1]) == 0
    assert heads_of(rb) == want
    rb.close()


def test_live_random_set():
    """about 2 000 texts of at most 200 bases against 8 members, made now: at least a third of the texts have a head and at least
    a third have none (asserted on the definition before the run), so a run cannot pass by reporting nothing -- or everything"""
    rng = np.random.default_rng(20261021)
    panel = [G.rand_seq(rng, int(m)) for m in rng.integers(18, 41, 8)]
    bounds = [int(b) for b in rng.integers(0, 5, 8)]
    texts = []
    for i in range(2000):
        n = int(rng.integers(1, 201))
        if i % 2:
            p = int(rng.integers(0, 8))
            m = len(panel[p])
            r = int(rng.integers(5, m))
            head = G.mutate(rng, panel[p][m - r:][::-1], int(rng.integers(0, (r * min(bounds[p], m)) // m + 1)))[::-1]      # (no edit at the first base)
            texts.append(G.start_with(rng, head, max(n, 8)))
        else:
            texts.append(G.rand_seq(rng, n))
    want = H.all_heads(texts, panel, bounds, 0, 3)
    have = sum(t[0] >= 0 for t in want)
    assert 3 * have >= len(want) and 3 * (len(want) - have) >= len(want), have
    rb = batch_of(texts)
    got = flagged_and_plain(rb, INFIX | TL, panel, bounds, 16)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, bad[:5]
    most_steps, most_rows = step_bounds(texts, panel, bounds)
    assert 0 < int(rb.counters()[6]) <= most_steps and 0 < int(rb.counters()[7]) <= most_rows
    rb.close()


def test_long_texts_walk_their_start_only():
    """64 texts of 5 000 bases against 8 members: the answers are the full matrix's, and counter [6] is within the short sweep's
    derived bound -- the sum over texts and members of blocks(m) min(n, m + k) --, which a kernel that walks the whole text fails"""
    rng = np.random.default_rng(20261022)
    lens = (18, 24, 33, 48, 64, 65, 100, 130)
    panel = [G.rand_seq(rng, m) for m in lens]
    bounds = [1, 2, 3, 4, 6, 6, 9, 12]
    texts = []
    for i in range(64):
        p = i % 8
        m = lens[p]
        r = int(rng.integers(8, m))
        head = G.mutate(rng, panel[p][m - r:][::-1], int(rng.integers(0, (r * bounds[p]) // m + 1)))[::-1] if i % 4 else b""
        texts.append(G.start_with(rng, head, 5000))
    want = H.all_heads(texts, panel, bounds, 0, 3)
    assert sum(t[0] >= 0 for t in want) >= 40
    rb = batch_of(texts)
    got = flagged_and_plain(rb, INFIX, panel, bounds, 16)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, bad[:5]
    most_steps, most_rows = step_bounds(texts, panel, bounds)
    assert most_steps == 64 * sum((m + 63) // 64 * (m + k) for m, k in zip(lens, bounds)) < 64 * 5000
    assert 0 < int(rb.counters()[6]) <= most_steps, (int(rb.counters()[6]), most_steps)
    assert 0 < int(rb.counters()[7]) <= most_rows
    rb.close()


def test_the_getter_refuses_after_a_run_without_the_bit_and_the_bit_is_refused_elsewhere():
    texts = [b"TCGGAAGAGCCTCTCTCT", b"CTCTCTCT"]
    panel = [b"AGATCGGAAGAGC"]
    hand = [(0, 10, 10, 0), H.NONE]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | HD, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert heads_of(rb) == hand
    c = rb.counters().copy()
    assert c[6] > 0 and c[7] > 0
    # refused with nothing launched: results, heads and counters stay
    assert rb.run_panel(INFIX | HD, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | HD, panel, 1, max_hits=4, window=64) == capi.QUICKED_ERROR
    for other in (128, 256, 1024, 4096, 16384):
        assert rb.run_panel_all(INFIX | HD | other, panel, 1, max_hits=4) == capi.QUICKED_ERROR
    assert rb.run_panel_all(PREFIX | HD | TL, panel, 1, max_hits=4) == capi.QUICKED_ERROR
    for bad in (0, -1, capi.PANEL_MAX_LEN + 1):
        assert rb.configure_panel_heads(bad) == capi.QUICKED_ERROR
    assert heads_of(rb) == hand and (rb.counters() == c).all()
    # min_overlap holds for the runs to come and leaves the tails' setting alone
    tails_at_3 = T.all_tails(texts, panel, [1], 0, 3)
    assert rb.configure_panel_heads(11) == capi.QUICKED_OK
    assert rb.run_panel_all(INFIX | HD | TL, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert heads_of(rb) == [H.NONE, H.NONE] and tails_of(rb) == tails_at_3
    assert rb.configure_panel_tails(12) == capi.QUICKED_OK and rb.configure_panel_heads(3) == capi.QUICKED_OK
    assert rb.run_panel_all(INFIX | HD | TL, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert heads_of(rb) == hand and tails_of(rb) == T.all_tails(texts, panel, [1], 0, 12)
    # PREFIX takes the bit: the heads' matrix is its own
    assert rb.run_panel_all(PREFIX | HD, panel, 1, max_hits=4) == capi.QUICKED_OK
    assert heads_of(rb) == hand
    # a run without the bit after a flagged run: the getter refuses
    assert rb.run_panel_all(INFIX, panel, 1, max_hits=4) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.panel_heads()
    assert rb.counters()[6] == 0 and rb.counters()[7] == 0
    rb.close()
