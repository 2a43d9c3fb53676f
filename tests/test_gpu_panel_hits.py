"""Panel search, every occurrence, on the GPU (quicked_batch_run_panel_all through capi.ResidentBatch.run_panel_all): per text,
every occurrence of every panel member.  Expected values never come from the library: tests/panel_hits_lib.py -- the per-pair
brute forces of the all-occurrences search, concatenated in (pattern, text_end) order and capped -- over the lists recorded in
tests/golden/panel_hits_cases.json (a sample of which tests/test_panel_hits_cpu.py recomputes), or computed live for the small
sets made here.  The one test at size compares the library's two routes with each other (the panel run against the n x K pair
batch through run_search_all, regrouped in numpy) and a fixed sample of its texts with panel_hits_lib."""
import importlib.util
import os

import numpy as np
import pytest

import panel_hits_lib as PH
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = capi.SEARCH_PREFIX, capi.SEARCH_INFIX
MODES = [PREFIX, INFIX]
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "2", "4096"]                 # QE_PANEL_SLICES: the host's choice, one, two, one per member
CAPS = [1, 2, 64]
ACGT = b"ACGT"


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_hits_cases")


@pytest.fixture(scope="module")
def sets():
    return G.load()


def _pool(seqs):
    pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    return pool, off, ln


def batch_of(texts, patterns=None, wire=None):
    """the texts as the texts of a batch whose own patterns are `patterns` (default: all empty)"""
    patterns = [b""] * len(texts) if patterns is None else patterns
    pp, po, pl = _pool(patterns)
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
    rows = np.stack([hits[f] for f in PH.OCC_FIELDS], axis=1).astype(np.int64).tolist() if len(hits) else []
    return found, stored, [[tuple(r) for r in rows[off[i]:off[i + 1]]] for i in range(len(found))]


def run_and_compare(rb, texts, panel, mode, flag, bounds, cap, want=None):
    """bounds: None (no bound), one int (through max_dist_all) or one per member; found, stored, every stored record, the
    scores getter, the statuses and the other getters' refusals.  want: the uncapped lists, if at hand"""
    if want is None:
        per_member = [PH.INT32_MAX if bounds is None else int(bounds)] * len(panel) if np.ndim(bounds) == 0 else [int(b) for b in bounds]
        want = PH.all_hits(texts, panel, per_member, mode, flag)
    arg = bounds if bounds is None or np.ndim(bounds) == 0 else np.asarray(bounds, dtype=np.int32)
    assert rb.run_panel_all(mode | flag, panel, arg, max_hits=cap) == capi.QUICKED_OK
    found, stored, got = got_lists(rb)
    exp = [PH.capped(h, cap) for h in want]
    bad = [(i, len(texts[i]), int(found[i]), got[i][:4], e[0], e[1][:4]) for i, e in enumerate(exp) if (int(found[i]), got[i]) != (e[0], e[1])]
    assert not bad, (mode, flag, cap, len(bad), bad[:4])
    sc, st = rb.scores()
    assert sc.tolist() == [e[2] for e in exp]
    assert st.tolist() == [capi.QUICKED_OK if t else capi.QUICKED_EMPTY_SEQUENCE for t in texts]
    assert all(c is None for c in rb.cigars())
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix):
        with pytest.raises(capi.QuickedException):
            getter()
    return want


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name", ["named", "random"])
def test_named_and_random_sets(sets, name, nslices, monkeypatch):
    s = sets[name]
    texts, panel = s["texts"], s["panel"]
    slices(monkeypatch, nslices)
    rb = batch_of(texts)
    for mode in MODES:
        for flag in FLAGS:
            for conf in G.CONFS:
                want = s["hits"][(mode, flag, conf)]
                for cap in CAPS:
                    rb.kernel_times()
                    run_and_compare(rb, texts, panel, mode, flag, s["bounds"] if conf == "own" else s["uniform"], cap, want)
                    _, launches = rb.kernel_times()
                    assert launches[0] >= (2 if mode == INFIX and any(want) else 1) and rb.counters()[0] > 0      # the passes: slot [0] of both
    rb.close()


def _rand(rng, n):
    return bytes(ACGT[int(x)] for x in rng.integers(0, 4, n))


def small_set(n, k, seed):
    """n texts of 20 .. 140 bases, each holding one or two of k members of 12 .. 80 bases with a few errors"""
    rng = np.random.default_rng(seed)
    panel = [_rand(rng, int(rng.integers(12, 81))) for _ in range(k)]
    texts = []
    for _ in range(n):
        pieces = [G.mutate(rng, panel[int(rng.integers(0, k))], 0.06) for _ in range(int(rng.integers(1, 3)))]
        texts.append(G.plant(rng, int(rng.integers(20, 141)), pieces))
    return texts, panel


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_partial_waves(n, monkeypatch):
    texts, panel = small_set(n, 5, 100 + n)
    rb = batch_of(texts)
    for mode in MODES:
        want = PH.all_hits(texts, panel, [6] * 5, mode, 0)
        for nslices in (None, "2"):
            slices(monkeypatch, nslices)
            for cap in (1, 64):
                run_and_compare(rb, texts, panel, mode, 0, 6, cap, want)
    rb.close()


def test_no_bound_is_the_member_length():
    """max_dist None: every member's bound is its own length -- every valley of row m counts"""
    texts, panel = small_set(6, 3, 321)
    rb = batch_of(texts)
    for mode in MODES:
        want = run_and_compare(rb, texts, panel, mode, 0, None, 4096)
        assert all(len(h) >= 3 for h in want)
    rb.close()


def test_the_batch_patterns_play_no_part(sets):
    s = sets["named"]
    texts, panel = s["texts"], s["panel"]
    rng = np.random.default_rng(9)
    long_patterns = [_rand(rng, 700 - 13 * (i % 40)) for i in range(len(texts))]
    for patterns in (None, long_patterns):
        rb = batch_of(texts, patterns)
        run_and_compare(rb, texts, panel, INFIX, 0, s["bounds"], 64, s["hits"][(INFIX, 0, "own")])
        rb.close()


@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches_equal_the_ascii_batch(sets, wire):
    s = sets["random"]
    ok = set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN")
    keep = [i for i, t in enumerate(s["texts"]) if t and set(t) <= ok]
    texts = [s["texts"][i] for i in keep]
    assert len(texts) >= 150
    patterns = [b"ACGT"] * len(texts)                  # (the wire packers take upper-case ACGT / N)
    rp, ra = batch_of(texts, patterns, wire=wire), batch_of(texts, patterns)
    for mode in MODES:
        for flag in FLAGS:
            want = [s["hits"][(mode, flag, "own")][i] for i in keep]
            res = []
            for rb in (rp, ra):
                assert rb.run_panel_all(mode | flag, s["panel"], s["bounds"], max_hits=64) == capi.QUICKED_OK
                res.append(got_lists(rb))
            assert res[0][0].tolist() == res[1][0].tolist() and res[0][2] == res[1][2], (mode, flag)
            assert res[0][0].tolist() == [len(h) for h in want] and res[0][2] == [h[:64] for h in want], (mode, flag)
    rp.close()
    ra.close()


def test_consequences_against_the_panel_run(sets):
    """1: the smallest key (score, pattern) and its first occurrence is the panel run's best, the smallest key among the other
    members its runner-up; 2: a member's smallest score and the first end that has it is the matrix entry"""
    for name in ("named", "random"):
        s = sets[name]
        texts, panel = s["texts"], s["panel"]
        k = len(panel)
        rb = batch_of(texts)
        for mode in MODES:
            for flag in (0, capi.SEARCH_IUPAC):
                for bounds in (s["bounds"], s["uniform"]):
                    arg = bounds if np.ndim(bounds) == 0 else np.asarray(bounds, dtype=np.int32)
                    assert rb.run_panel_all(mode | flag, panel, arg, max_hits=4096) == capi.QUICKED_OK
                    found, stored, got = got_lists(rb)
                    assert np.array_equal(found, stored)
                    assert rb.run_panel(mode | flag, panel, arg, matrix=True) == capi.QUICKED_OK
                    r = rb.panel_results()
                    ms, me = rb.panel_matrix()
                    for i in range(len(texts)):
                        assert PH.best_two(got[i]) == tuple(int(r[i][f]) for f in ("pattern", "score", "text_start", "text_end", "second_pattern", "second_score")), (name, mode, flag, i)
                        assert PH.member_best(got[i], k) == (ms[i].tolist(), me[i].tolist()), (name, mode, flag, i)
        rb.close()


def regroup_pairs(found, off, hits, n, k, cap):
    """the n x K pair batch's lists (pair i K + p: member p against text i) -> per text (found, the first cap of [(pattern,
    text_start, text_end, score)]): pair order within a text is member order, each pair's list is ordered by text_end"""
    counts = np.diff(off)
    pattern = np.repeat(np.arange(n * k) % k, counts)
    rows = np.stack([pattern, hits["text_start"], hits["text_end"], hits["score"]], axis=1).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum(counts.reshape(n, k).sum(axis=1))])
    return found.reshape(n, k).sum(axis=1), [[tuple(r) for r in rows[toff[i]:toff[i + 1]][:cap].tolist()] for i in range(n)]


def test_route_agreement_at_size():
    """2 000 texts of 150 bases x 24 members of 20 .. 40 bases: the panel run against the library's pairwise route"""
    rng = np.random.default_rng(78)
    n, k, cap, bound = 2000, 24, 8, 5
    panel = [_rand(rng, int(rng.integers(20, 41))) for _ in range(k)]
    panel[5] = panel[4]                                            # a duplicate
    codes = rng.integers(0, 4, (n, 150)).astype(np.uint8)
    tarr = np.frombuffer(ACGT, dtype=np.uint8)[codes]
    for i in range(n):
        at = 0
        for _ in range(i % 4):                                     # 0 .. 3 members per text, the same one twice now and then
            q = G.mutate(rng, panel[int(rng.integers(0, 8 if i % 8 < 4 else k))], 0.08)
            if at + len(q) > 150:
                break
            at = int(rng.integers(at, 150 - len(q) + 1))
            tarr[i, at:at + len(q)] = np.frombuffer(q, dtype=np.uint8)
            at += len(q)
    texts = [tarr[i].tobytes() for i in range(n)]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX, panel, bound, max_hits=cap) == capi.QUICKED_OK
    found, stored, got = got_lists(rb)
    rb.close()
    # the pairwise route: pair i * K + p is member p against text i; the same cap keeps at least a text's first `cap`
    pp, po, pl = _pool(panel * n)
    tp = np.repeat(tarr, k, axis=0).reshape(-1)
    tl = np.full(n * k, 150, dtype=np.int32)
    to = (np.arange(n * k, dtype=np.int64) * 150)
    rq = capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl))
    assert rq.run_search_all(INFIX, bound, max_hits=cap) == capi.QUICKED_OK
    pfound, poff, phits = rq.hits()
    rq.close()
    wfound, want = regroup_pairs(pfound, poff, phits, n, k, cap)
    assert found.tolist() == wfound.tolist()
    assert stored.tolist() == np.minimum(wfound, cap).tolist()
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (len(bad), [(i, got[i], want[i]) for i in bad[:4]])
    assert int((found >= 2).sum()) > n // 4 and int((found == 0).sum()) > n // 50
    sample = [int(i) for i in np.random.default_rng(3).choice(n, 200, replace=False)]
    exp = [PH.capped(h, cap) for h in PH.all_hits([texts[i] for i in sample], panel, [bound] * k, INFIX, 0)]
    assert [(int(found[i]), got[i]) for i in sample] == [(e[0], e[1]) for e in exp]


def test_panel_panel_all_and_search_all_runs_in_turn(sets):
    s = sets["named"]
    texts, panel = s["texts"], s["panel"]
    patterns = [panel[i % len(panel)] for i in range(len(texts))]
    rb = batch_of(texts, patterns)
    for getter in (rb.panel_hits, rb.panel_hit_counts):
        with pytest.raises(capi.QuickedException):
            getter()
    for _ in range(2):
        assert rb.run_panel(INFIX, panel, s["uniform"]) == capi.QUICKED_OK
        rb.panel_results()
        for getter in (rb.panel_hits, rb.panel_hit_counts, rb.hits):
            with pytest.raises(capi.QuickedException):
                getter()
        run_and_compare(rb, texts, panel, INFIX, 0, s["uniform"], 2, s["hits"][(INFIX, 0, "uniform")])
        assert rb.run_search_all(INFIX, 10, max_hits=4) == capi.QUICKED_OK
        pfound, poff, phits = rb.hits()
        for i, (q, t) in enumerate(zip(patterns, texts)):
            occ = PH.occurrences(q, t, INFIX, 0, 10) if t else []
            assert int(pfound[i]) == len(occ) and [tuple(int(x) for x in h) for h in phits[poff[i]:poff[i + 1]]] == occ[:4], i
        for getter in (rb.panel_hits, rb.panel_hit_counts, rb.panel_results):
            with pytest.raises(capi.QuickedException):
                getter()
    rb.close()


def test_argument_rules_on_the_device(sets):
    s = sets["named"]
    rb = batch_of(s["texts"][:8])
    panel = s["panel"]
    assert rb.run_panel_all(INFIX, panel, 3) == capi.QUICKED_OK
    before = got_lists(rb)
    cnt = rb.counters()[0]
    assert rb.run_panel_all(INFIX | capi.SEARCH_IUPAC | capi.SEARCH_IUPAC_PATTERN, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | capi.PANEL_MATRIX, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(3, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, panel + [b""], 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, panel, -1) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, panel, 3, max_hits=0) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, panel, 3, max_hits=4097) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, [b"ACGT"] * 4097, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX, panel + [b"A" * 257], 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX, panel, 3, sync=False) == capi.QUICKED_UNIMPLEMENTED
    after = got_lists(rb)
    assert after[0].tolist() == before[0].tolist() and after[2] == before[2] and rb.counters()[0] == cnt      # nothing ran
    rb.close()
