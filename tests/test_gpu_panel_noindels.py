"""Panel search by mismatches only, on the GPU (QUICKED_PANEL_NO_INDELS through capi.ResidentBatch.run_panel and run_panel_all).
Expected values never come from the library: tests/panel_noindels_lib.py -- plain loops over bytes, the three equalities written
out there -- over the results recorded in tests/golden/panel_noindels_cases.json (a sample of which
tests/test_panel_noindels_cpu.py recomputes), or computed live for the set at size.  Every field is compared: the six fields of
every text's record, the matrix, found / stored, every stored occurrence, the scores, the statuses, counter [0]."""
import importlib.util
import os

import numpy as np
import pytest

import panel_noindels_lib as N
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX, NI = capi.SEARCH_PREFIX, capi.SEARCH_INFIX, capi.PANEL_NO_INDELS
MODES = [PREFIX, INFIX]
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "4096"]                      # QE_PANEL_SLICES: the host's choice, one, one per member
WIRES = [None, capi.WIRE_2BIT, capi.WIRE_PLANES3]
GROUPS = ["lengths", "homopolymer", "indels", "single", "bytes", "panel130", "wave65"]
ACGT = b"ACGT"


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_noindels_cases")


@pytest.fixture(scope="module")
def groups():
    return _RECORD


def _pool(seqs):
    pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    return pool, off, ln


def batch_of(texts, wire=None):
    """the texts as the texts of a batch whose own patterns play no part (empty; ACGT where a wire packer reads them)"""
    pp, po, pl = _pool([b"ACGT" if wire is not None else b""] * len(texts))
    tp, to, tl = _pool(texts)
    return capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl), wire=wire)


def slices(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("QE_PANEL_SLICES", raising=False)
    else:
        monkeypatch.setenv("QE_PANEL_SLICES", value)


def got_lists(rb):
    """-> (found, stored, per text [(pattern, text_start, text_end, score)])"""
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    assert hits.dtype == capi.PANEL_OCC_DTYPE and off[0] == 0 and off[-1] == len(hits)
    assert np.array_equal(np.diff(off), stored)
    rows = np.stack([hits[f] for f in N.OCC_FIELDS], axis=1).astype(np.int64).tolist() if len(hits) else []
    return found, stored, [[tuple(r) for r in rows[off[i]:off[i + 1]]] for i in range(len(found))]


def got_records(rb):
    r = rb.panel_results()
    return [tuple(int(r[i][f]) for f in N.HIT_FIELDS) for i in range(len(r))]


def check_best(rb, texts, panel, bounds, mode, flag, D, E, matrix):
    """one flagged run_panel against the matrix rows D / E of these texts"""
    rb.kernel_times()
    assert rb.run_panel(mode | flag | NI, panel, np.asarray(bounds, dtype=np.int32), matrix=matrix) == capi.QUICKED_OK
    want = [N.reduce_text(D[i], E[i], panel) for i in range(len(texts))]
    got = got_records(rb)
    bad = [(i, got[i], want[i]) for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (mode, flag, len(bad), bad[:4])
    sc, st = rb.scores()
    assert sc.tolist() == [w[1] for w in want]
    assert st.tolist() == [capi.QUICKED_OK if t else capi.QUICKED_EMPTY_SEQUENCE for t in texts]
    if matrix:
        ms, me = rb.panel_matrix()
        assert ms.tolist() == [list(r) for r in D] and me.tolist() == [list(r) for r in E], (mode, flag)
    else:
        with pytest.raises(capi.QuickedException):
            rb.panel_matrix()
    counters = rb.counters()
    assert int(counters[0]) == N.block_steps(texts, panel, mode) and not any(int(c) for c in counters[1:]), (mode, flag, counters)
    _, launches = rb.kernel_times()
    assert launches[0] == 1 and not any(launches[1:])                      # the sweep alone: no start pass
    for getter in (rb.panel_hits, rb.panel_hit_counts, rb.locations, rb.hits):
        with pytest.raises(capi.QuickedException):
            getter()


def check_all(rb, texts, panel, bounds, mode, flag, found_want, occ_want, best_want, cap):
    """one flagged run_panel_all: occ_want holds at least the first `cap` occurrences of every text"""
    rb.kernel_times()
    assert rb.run_panel_all(mode | flag | NI, panel, np.asarray(bounds, dtype=np.int32), max_hits=cap) == capi.QUICKED_OK
    found, stored, got = got_lists(rb)
    bad = [(i, int(found[i]), got[i][:3], found_want[i], occ_want[i][:3]) for i in range(len(texts))
           if (int(found[i]), got[i]) != (found_want[i], [tuple(o) for o in occ_want[i][:cap]])]
    assert not bad, (mode, flag, cap, len(bad), bad[:4])
    assert stored.tolist() == [min(f, cap) for f in found_want]
    sc, st = rb.scores()
    assert sc.tolist() == best_want
    assert st.tolist() == [capi.QUICKED_OK if t else capi.QUICKED_EMPTY_SEQUENCE for t in texts]
    counters = rb.counters()
    assert int(counters[0]) == N.block_steps(texts, panel, mode) and not any(int(c) for c in counters[1:]), (mode, flag, counters)
    _, launches = rb.kernel_times()
    assert launches[0] == 1 and not any(launches[1:])
    assert all(c is None for c in rb.cigars())
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix, rb.panel_hit_cigars, rb.panel_tails, rb.panel_heads):
        with pytest.raises(capi.QuickedException):
            getter()


def fitting(texts, wire):
    """the texts a wire format can carry: all of them as ASCII, upper-case ACGT as 2BIT, with N as PLANES3"""
    ok = None if wire is None else (set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN"))
    return [i for i, t in enumerate(texts) if ok is None or (t and set(t) <= ok)]


# every group over every wire that carries at least one of its texts (the `bytes` group has no text of upper-case ACGT alone)
_RECORD = G.load()
GROUP_WIRES = [(name, wire) for name in GROUPS for wire in WIRES if fitting(_RECORD[name]["texts"], wire)]
assert len(GROUP_WIRES) == 3 * len(GROUPS) - 1 and ("bytes", capi.WIRE_PLANES3) in GROUP_WIRES


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name,wire", GROUP_WIRES)
def test_the_fixture_through_both_runs(groups, name, nslices, wire, monkeypatch):
    g = groups[name]
    keep = fitting(g["texts"], wire)
    texts, panel, bounds = [g["texts"][i] for i in keep], g["panel"], g["bounds"]
    slices(monkeypatch, nslices)
    rb = batch_of(texts, wire)
    for mode in MODES:
        for flag in FLAGS:
            r = g["results"][(mode, flag)]
            D, E = [r["d"][i] for i in keep], [r["e"][i] for i in keep]
            for matrix in (False, True):
                check_best(rb, texts, panel, bounds, mode, flag, D, E, matrix)
            best = [min([d for d in row if d >= 0], default=-1) for row in D]
            for cap in (1, 2, G.CAP):
                check_all(rb, texts, panel, bounds, mode, flag, [r["found"][i] for i in keep], [r["occ"][i] for i in keep], best, cap)
    rb.close()


@pytest.mark.parametrize("count", [1, 64, 65])
def test_batches_of_one_text_one_wave_and_a_wave_and_a_lane(groups, count):
    g = groups["wave65"]
    texts, panel, bounds = g["texts"][:count], g["panel"], g["bounds"]
    assert any(texts) and len({len(t) for t in texts}) >= min(count, 6)
    rb = batch_of(texts)
    for mode in MODES:
        r = g["results"][(mode, 0)]
        check_best(rb, texts, panel, bounds, mode, 0, r["d"][:count], r["e"][:count], True)
        best = [min([d for d in row if d >= 0], default=-1) for row in r["d"][:count]]
        check_all(rb, texts, panel, bounds, mode, 0, r["found"][:count], r["occ"][:count], best, G.CAP)
    rb.close()


def test_consequences_between_the_two_flagged_runs(groups):
    """1: the smallest key (score, pattern) with its first occurrence is the flagged run_panel's record, the smallest key among
    the other members its runner-up; 2: a member's smallest score and the first end that has it is the flagged matrix entry"""
    for name in GROUPS:
        g = groups[name]
        texts, panel, k = g["texts"], g["panel"], len(g["panel"])
        bounds = np.asarray(g["bounds"], dtype=np.int32)
        rb = batch_of(texts)
        for mode in MODES:
            for flag in FLAGS:
                assert rb.run_panel_all(mode | flag | NI, panel, bounds, max_hits=4096) == capi.QUICKED_OK
                found, stored, got = got_lists(rb)
                assert np.array_equal(found, stored)
                assert rb.run_panel(mode | flag | NI, panel, bounds, matrix=True) == capi.QUICKED_OK
                rec = got_records(rb)
                ms, me = rb.panel_matrix()
                for i in range(len(texts)):
                    assert N.best_two(got[i]) == rec[i], (name, mode, flag, i)
                    assert N.member_best(got[i], k) == (ms[i].tolist(), me[i].tolist()), (name, mode, flag, i)
        rb.close()


def test_with_every_bound_zero_both_definitions_agree(groups):
    """an exact match is an exact match under both definitions: identical records, matrix and occurrences"""
    seen = 0
    for name in GROUPS:
        g = groups[name]
        texts, panel = g["texts"], g["panel"]
        rb = batch_of(texts)
        for mode in MODES:
            for flag in FLAGS:
                res = []
                for bit in (0, NI):
                    assert rb.run_panel(mode | flag | bit, panel, 0, matrix=True) == capi.QUICKED_OK
                    rec, (ms, me) = got_records(rb), rb.panel_matrix()
                    assert rb.run_panel_all(mode | flag | bit, panel, 0, max_hits=64) == capi.QUICKED_OK
                    found, stored, got = got_lists(rb)
                    res.append((rec, ms.tolist(), me.tolist(), found.tolist(), got))
                assert res[0] == res[1], (name, mode, flag)
                seen += sum(res[1][3])
        rb.close()
    assert seen > 100


def _rand(rng, n):
    return bytes(ACGT[int(x)] for x in rng.integers(0, 4, n))


def test_one_set_at_size():
    """2 000 random texts of 40 .. 200 bases, a third with a planted member carrying 0 .. 3 substitutions, against 40 members
    of 16 .. 70 bases, bound 2: against the loops of panel_noindels_lib.py, computed live (H_batch: the same count with the loop
    over the texts in numpy, held to the plain loops by tests/test_panel_noindels_cpu.py)"""
    rng = np.random.default_rng(2026)
    n, k, bound, cap = 2000, 40, 2, 8
    panel = [_rand(rng, int(rng.integers(16, 71))) for _ in range(k)]
    texts = []
    for i in range(n):
        length = int(rng.integers(40, 201))
        if i % 3 == 0:
            q = G.substitute(rng, panel[int(rng.integers(0, k))], int(rng.integers(0, 4)))
            texts.append(G.plant(rng, max(length, len(q)), q))
        else:
            texts.append(_rand(rng, length))
    assert all(40 <= len(t) <= 200 for t in texts)
    D = np.full((n, k), -1, dtype=np.int64)
    E = np.full((n, k), -1, dtype=np.int64)
    hits = [[] for _ in range(n)]
    for p, q in enumerate(panel):
        H = N.H_batch(q, texts, 0)
        m = len(q)
        for i in np.nonzero(((H >= 0) & (H <= bound)).any(axis=1))[0]:
            i = int(i)
            R = {s + m: int(v) for s, v in enumerate(H[i]) if v >= 0}
            D[i, p], E[i, p] = N.best_of(R, bound)
            hits[i] += [(p, e - m, e, v) for e, v in N.valleys_of(R, bound)]
    within = int((D >= 0).sum())
    assert n // 5 < within < n, within                           # the planted members within 2, and few others
    bounds = [bound] * k
    rb = batch_of(texts)
    check_best(rb, texts, panel, bounds, INFIX, 0, D.tolist(), E.tolist(), True)
    best = [min([int(d) for d in row if d >= 0], default=-1) for row in D]
    check_all(rb, texts, panel, bounds, INFIX, 0, [len(h) for h in hits], hits, best, cap)
    rb.close()


def test_refusals_through_the_c_abi(groups):
    g = groups["indels"]
    panel = g["panel"]
    rb = batch_of(g["texts"])
    assert rb.run_panel_all(INFIX | NI, panel, 1) == capi.QUICKED_OK
    before, cnt = got_lists(rb), rb.counters()[0]
    CG, TL, HD = capi.PANEL_CIGARS, capi.PANEL_TAILS, capi.PANEL_HEADS
    # the QUICKED_ERROR rules come first, unchanged; on the other runs the bit is an unknown bit
    for extra in (4, 8, 128, 256, 1024, 4096, 16384, 65536, capi.SEARCH_IUPAC | capi.SEARCH_IUPAC_PATTERN):
        assert rb.run_panel(INFIX | NI | extra, panel, 1) == capi.QUICKED_ERROR
        assert rb.run_panel_all(INFIX | NI | extra, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel(NI, panel, 1) == capi.QUICKED_ERROR and rb.run_panel(3 | NI, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | NI | capi.PANEL_MATRIX, panel, 1) == capi.QUICKED_ERROR
    for bit in (CG, TL, HD):
        assert rb.run_panel(INFIX | NI | bit, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel_all(PREFIX | NI | TL, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | NI, panel, -1) == capi.QUICKED_ERROR and rb.run_panel(INFIX | NI, panel + [b""], 1) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | NI, panel, 1, max_hits=0) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | NI, panel, 1, max_hits=4097, sync=False) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | NI, panel, 1) == capi.QUICKED_ERROR
    assert rb.run_search(INFIX | NI, 1) == capi.QUICKED_ERROR and rb.run_search_all(INFIX | NI, 1) == capi.QUICKED_ERROR
    # QUICKED_UNIMPLEMENTED with the bit, nothing launched
    for mode in MODES:
        assert rb.run_panel_all(mode | NI | CG, panel, 1) == capi.QUICKED_UNIMPLEMENTED
        assert rb.run_panel_all(mode | NI | HD, panel, 1) == capi.QUICKED_UNIMPLEMENTED
        assert rb.run_panel_all(mode | NI, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
        assert rb.run_panel(mode | NI, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | NI | TL, panel, 1) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | NI | TL | HD | CG, panel, 1) == capi.QUICKED_UNIMPLEMENTED
    rb.configure_panel_queue(1 << 16)                                 # ... also on a batch object whose queue is switched on
    assert rb.run_panel_all(INFIX | NI, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel(INFIX | NI | capi.SEARCH_IUPAC, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
    rb.configure_panel_queue(0)
    assert rb.run_panel(INFIX | NI, panel + [b"A" * 257], 1) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | NI, panel + [b"A" * 257], 1) == capi.QUICKED_UNIMPLEMENTED
    rb.configure(check=1)
    assert rb.run_panel(INFIX | NI, panel, 1) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | NI, panel, 1) == capi.QUICKED_UNIMPLEMENTED
    rb.configure(check=0)
    after = got_lists(rb)
    assert after[0].tolist() == before[0].tolist() and after[2] == before[2] and rb.counters()[0] == cnt      # nothing ran
    rb.close()
