"""Queued panel runs on the GPU (quicked_batch_configure_panel_queue; run_panel and run_panel_all with sync=False, then fetch()).
Expected values never come from the library's sync run alone: they are the definitions' (tests/panel_queue_lib.py over
panel_lib, panel_hits_lib, panel_tails_lib and panel_heads_lib) on the named and random sets of the four recorded panel
fixtures, or computed live for the small sets made here; the overflow rule is restated there (capped_run).  Beside the
definitions a roomy queued run is held against the sync run of the same batch where the issue is "bit for bit": counter [0]."""
import numpy as np
import pytest

import panel_queue_lib as Q
import panel_hits_lib as PH
import panel_heads_lib as H
import panel_tails_lib as T
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

PREFIX, INFIX, TL, HD = capi.SEARCH_PREFIX, capi.SEARCH_INFIX, capi.PANEL_TAILS, capi.PANEL_HEADS
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "4096"]
ROOMY = 1 << 20
OK, EMPTY = capi.QUICKED_OK, capi.QUICKED_EMPTY_SEQUENCE


def _pool(seqs):
    pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    return pool, off, ln


def batch_of(texts, wire=None, max_total=ROOMY, patterns=None):
    pp, po, pl = _pool([b""] * len(texts) if patterns is None else patterns)
    tp, to, tl = _pool(texts)
    rb = capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl), wire=wire)
    if max_total is not None:
        assert rb.configure_panel_queue(max_total) == OK
    return rb


def env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def fields(a, names):
    return [tuple(int(a[f][i]) for f in names) for i in range(len(a))]


def check_best(rb, texts, want):
    """the fetched results of a queued run_panel: every field of every text, scores, statuses, the other getters' refusals"""
    got = fields(rb.panel_results(), Q.P.HIT_FIELDS)
    bad = [(i, a, tuple(b)) for i, (a, b) in enumerate(zip(got, want)) if a != tuple(b)]
    assert not bad, bad[:5]
    sc, st = rb.scores()
    assert sc.tolist() == [w[1] for w in want]
    assert st.tolist() == [OK if t else EMPTY for t in texts]
    assert rb.panel_queue_wanted() == -1
    for getter in (rb.locations, rb.hits, rb.panel_matrix, rb.panel_hits, rb.panel_hit_counts, rb.panel_tails, rb.panel_heads):
        with pytest.raises(capi.QuickedException):
            getter()


def check_all(rb, texts, lists, cap, max_total, tails=None, heads=None):
    """the fetched results of a queued run_panel_all against the uncapped lists: found, scores, statuses, tails and heads exact
    whatever the room; the records the first max_total of the array; hit_off' and stored'; wanted == W.  -> W"""
    found, off, recs, scores, W = Q.capped_run(lists, cap, max_total)
    gf, gs = rb.panel_hit_counts()
    goff, hits = rb.panel_hits()
    got = fields(hits, PH.OCC_FIELDS)
    assert gf.tolist() == found
    assert goff.tolist() == off and gs.tolist() == np.diff(off).tolist()
    assert len(got) == min(W, max_total) and got == recs, [(j, a, b) for j, (a, b) in enumerate(zip(got, recs)) if a != b][:5]
    assert rb.panel_queue_wanted() == W
    sc, st = rb.scores()
    assert sc.tolist() == scores
    assert st.tolist() == [OK if t else EMPTY for t in texts]
    if tails is None:
        with pytest.raises(capi.QuickedException):
            rb.panel_tails()
    else:
        assert fields(rb.panel_tails(), T.TAIL_FIELDS) == [tuple(t) for t in tails]
    if heads is None:
        with pytest.raises(capi.QuickedException):
            rb.panel_heads()
    else:
        assert fields(rb.panel_heads(), H.HEAD_FIELDS) == [tuple(t) for t in heads]
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix, rb.panel_hit_cigars):
        with pytest.raises(capi.QuickedException):
            getter()
    return W


def queued(rb, run, *args, **kw):
    assert run(*args, sync=False, **kw) == OK
    assert rb.fetch() == OK


def bounds_arg(g):
    return np.asarray(g["bounds"], dtype=np.int32)


# ---- the definition sets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name", ["named", "random"])
@pytest.mark.parametrize("fixture", ["search_panel", "panel_hits"])
def test_queued_run_panel_is_the_definition(fixture, name, nslices, monkeypatch):
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    for g in Q.groups(fixture, name):
        rb = batch_of(g["texts"])
        for mode in (PREFIX, INFIX):
            for flag in FLAGS:
                queued(rb, rb.run_panel, mode | flag, g["panel"], bounds_arg(g))
                check_best(rb, g["texts"], Q.best(g, mode, flag))
                c0 = int(rb.counters()[0])
                assert rb.run_panel(mode | flag, g["panel"], bounds_arg(g)) == OK and int(rb.counters()[0]) == c0 > 0
        rb.close()


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name", ["named", "random"])
@pytest.mark.parametrize("fixture", ["panel_hits", "panel_tails", "panel_heads"])
def test_queued_run_panel_all_is_the_definition(fixture, name, nslices, monkeypatch):
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    ran = 0
    for g in Q.groups(fixture, name):
        rb = batch_of(g["texts"])
        arg = bounds_arg(g)
        for mode in (PREFIX, INFIX):
            for flag in FLAGS:
                lists = Q.hits(g, mode, flag)
                for cap in (1, 2, 64):
                    assert rb.run_panel_all(mode | flag, g["panel"], arg, max_hits=cap) == OK
                    sync0 = int(rb.counters()[0])
                    assert rb.panel_queue_wanted() == -1
                    queued(rb, rb.run_panel_all, mode | flag, g["panel"], arg, max_hits=cap)
                    check_all(rb, g["texts"], lists, cap, ROOMY)
                    assert int(rb.counters()[0]) == sync0 > 0          # roomy: the block steps of the sync run
                    ran += 1
        rb.close()
    assert ran >= 18


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("fixture", ["panel_tails", "panel_heads"])
def test_queued_tails_and_heads_are_the_definition(fixture, nslices, monkeypatch):
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    ran = 0
    for g in Q.groups(fixture, "named") + Q.groups(fixture, "random"):
        rb = batch_of(g["texts"])
        arg = bounds_arg(g)
        for flag in FLAGS:
            for mo in (1, 3):
                assert rb.configure_panel_tails(mo) == OK and rb.configure_panel_heads(4 - mo) == OK      # (each its own)
                tails, heads = Q.tails(g, flag, mo), Q.heads(g, flag, 4 - mo)
                for mode, bits in ((INFIX, TL), (INFIX, HD), (INFIX, TL | HD), (PREFIX, HD)):
                    assert rb.run_panel_all(mode | flag | bits, g["panel"], arg, max_hits=64) == OK
                    sync = [int(c) for c in rb.counters()]
                    queued(rb, rb.run_panel_all, mode | flag | bits, g["panel"], arg, max_hits=64)
                    check_all(rb, g["texts"], Q.hits(g, mode, flag), 64, ROOMY, tails if bits & TL else None, heads if bits & HD else None)
                    got = [int(c) for c in rb.counters()]
                    assert [got[q] for q in (0, 2, 6, 7)] == [sync[q] for q in (0, 2, 6, 7)]
                    ran += 1
        rb.close()
    assert ran >= 150


@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches(wire):
    g = Q.groups("panel_hits", "random")[0]
    ok = set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN")
    keep = [i for i, t in enumerate(g["texts"]) if t and set(t) <= ok]
    texts = [g["texts"][i] for i in keep]
    assert len(texts) >= 150
    rb = batch_of(texts, wire=wire, patterns=[b"ACGT"] * len(texts))      # (the wire packers take upper-case ACGT / N)
    for mode in (PREFIX, INFIX):
        for flag in FLAGS:
            lists = [Q.hits(g, mode, flag)[i] for i in keep]
            heads = Q._cached(g, ("wire heads", wire, flag), lambda: H.all_heads(texts, g["panel"], g["bounds"], flag, 3))
            for cap in (1, 2, 64):
                queued(rb, rb.run_panel_all, mode | flag | HD, g["panel"], bounds_arg(g), max_hits=cap)
                check_all(rb, texts, lists, cap, ROOMY, None, heads)
            queued(rb, rb.run_panel, mode | flag, g["panel"], bounds_arg(g))
            check_best(rb, texts, [PH.best_two(h) for h in lists])
    rb.close()


# ---- shapes where the new code can go wrong ----------------------------------------------------------------------------------
ACGT = b"ACGT"


def _rand(rng, n, letters=ACGT):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), n))


def small_set(n, k, seed, empty_every=0):
    """n texts of 20 .. 140 bases, each holding one or two of k members of 12 .. 40 bases with an error now and then, every
    other text beginning with one (PREFIX); every empty_every-th text empty"""
    rng = np.random.default_rng(seed)
    panel = [_rand(rng, int(rng.integers(12, 41))) for _ in range(k)]
    texts = []
    for i in range(n):
        t = b"" if i % 2 == 0 else _rand(rng, int(rng.integers(5, 40)))
        for _ in range(int(rng.integers(1, 3))):
            q = bytearray(panel[int(rng.integers(0, k))])
            if rng.integers(0, 2):
                q[int(rng.integers(0, len(q)))] = ACGT[int(rng.integers(0, 4))]
            t += bytes(q) + _rand(rng, int(rng.integers(0, 30)))
        texts.append(b"" if empty_every and i % empty_every == 1 else t[:140])
    return texts, panel


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_partial_waves_with_empty_texts_and_small_rooms(n, monkeypatch):
    """1, 63, 64, 65 and 130 texts, every fifth empty; the room below 64, not a multiple of 64, exactly W, and roomy"""
    texts, panel = small_set(n, 5, 700 + n, empty_every=5 if n > 1 else 0)
    rb = batch_of(texts)
    for mode in (PREFIX, INFIX):
        lists = PH.all_hits(texts, panel, [3] * 5, mode, 0)
        W = Q.capped_run(lists, 4, ROOMY)[4]
        assert W >= (1 if n == 1 else n // 4)
        for nslices in (None, "2"):
            env(monkeypatch, "QE_PANEL_SLICES", nslices)
            for room in sorted({1, min(W, 37), min(W, 100), W, ROOMY}):
                assert rb.configure_panel_queue(room) == OK
                queued(rb, rb.run_panel_all, mode, panel, 3, max_hits=4)
                assert check_all(rb, texts, lists, 4, room) == W
        queued(rb, rb.run_panel, mode, panel, 3)
        check_best(rb, texts, [PH.best_two(h) for h in lists])
    rb.close()


def test_all_texts_empty():
    """nothing to launch: the queued run answers as the sync run does, and the fetch shows what the sync run leaves"""
    texts, panel = [b""] * 5, [b"ACGTACGT", b"TTTTGGGG"]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | HD, panel, 2, max_hits=4) == EMPTY
    found, stored = rb.panel_hit_counts()
    assert found.tolist() == stored.tolist() == [0] * 5
    assert rb.run_panel(INFIX, panel, 2) == EMPTY
    sync_best = fields(rb.panel_results(), Q.P.HIT_FIELDS)
    assert sync_best == [(-1,) * 6] * 5
    assert rb.run_panel_all(INFIX | HD, panel, 2, max_hits=4, sync=False) == EMPTY
    assert fields(rb.panel_results(), Q.P.HIT_FIELDS) == sync_best              # until the fetch
    assert rb.fetch() == OK
    found, stored = rb.panel_hit_counts()
    assert found.tolist() == stored.tolist() == [0] * 5 and len(rb.panel_hits()[1]) == 0 and rb.panel_queue_wanted() == 0
    assert rb.scores()[1].tolist() == [EMPTY] * 5
    assert rb.run_panel(INFIX, panel, 2, sync=False) == EMPTY and rb.fetch() == OK
    assert fields(rb.panel_results(), Q.P.HIT_FIELDS) == sync_best and rb.panel_queue_wanted() == -1
    rb.close()


def test_a_batch_without_an_occurrence():
    """W = 0: the room is taken and every lane of the start pass leaves at once; tails and heads are there all the same"""
    rng = np.random.default_rng(5)
    adapter = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    texts = [adapter[-(5 + i % 20):] + _rand(rng, 60 + i, b"CT") + adapter[:4 + i % 9] for i in range(130)] + [b""]
    rb = batch_of(texts)
    for mode, bits in ((INFIX, TL | HD), (INFIX, 0), (PREFIX, HD)):
        lists = PH.all_hits(texts, [adapter], [2], mode, 0)
        assert not any(lists)
        queued(rb, rb.run_panel_all, mode | bits, [adapter], 2, max_hits=4)
        W = check_all(rb, texts, lists, 4, ROOMY, T.all_tails(texts, [adapter], [2], 0, 3) if bits & TL else None,
                      H.all_heads(texts, [adapter], [2], 0, 3) if bits & HD else None)
        assert W == 0 and int(rb.counters()[0]) > 0
    rb.close()


# ---- overflow ----------------------------------------------------------------------------------------------------------------
def test_overflow_keeps_the_first_max_total_records():
    g = {x["name"]: x for x in Q.groups("panel_heads", "named")}["edges"]      # 13 texts, 3 members: W = 6 (INFIX) and 5 (PREFIX) at max_hits 2
    texts, panel, arg = g["texts"], g["panel"], bounds_arg(g)
    tails, heads = Q.tails(g, 0, 3), Q.heads(g, 0, 3)
    for mode in (INFIX, PREFIX):
        lists = Q.hits(g, mode, 0)
        W = Q.capped_run(lists, 2, ROOMY)[4]
        assert W > 4
        rb = batch_of(texts)
        assert rb.run_panel_all(mode, panel, arg, max_hits=2) == OK
        steps = int(rb.counters()[0])
        for room in (1, 2, W - 1, W, W + 1):
            assert rb.configure_panel_queue(room) == OK
            bits = (TL | HD) if mode == INFIX else HD
            queued(rb, rb.run_panel_all, mode | bits, panel, arg, max_hits=2)
            assert check_all(rb, texts, lists, 2, room, tails if bits & TL else None, heads) == W
            got = int(rb.counters()[0])
            assert got == steps if room >= W or mode == PREFIX else 0 < got < steps      # the block steps really walked
        rb.close()


# ---- several in flight ---------------------------------------------------------------------------------------------------------
def test_six_batches_queued_back_to_back_and_fetched_in_reverse():
    sets = [small_set(40 + 30 * q, 2 + q, 900 + q, empty_every=7) for q in range(6)]
    rbs = [batch_of(texts) for texts, _ in sets]
    for q, (rb, (texts, panel)) in enumerate(zip(rbs, sets)):
        run = rb.run_panel if q % 2 else rb.run_panel_all
        assert run(INFIX | (0 if q % 2 else HD), list(panel), 2 + q % 3, sync=False, **({} if q % 2 else {"max_hits": 3})) == OK
    for q in reversed(range(6)):
        texts, panel = sets[q]
        lists = PH.all_hits(texts, panel, [2 + q % 3] * len(panel), INFIX, 0)
        assert rbs[q].fetch() == OK
        if q % 2:
            check_best(rbs[q], texts, [PH.best_two(h) for h in lists])
        else:
            check_all(rbs[q], texts, lists, 3, ROOMY, None, H.all_heads(texts, panel, [2 + q % 3] * len(panel), 0, 3))
    for rb in rbs:
        rb.close()


def test_the_second_queued_run_supersedes_and_the_getters_wait_for_the_fetch():
    texts, panel = small_set(100, 4, 41, empty_every=9)
    other = small_set(1, 3, 42)[1]
    rb = batch_of(texts)
    assert rb.run_panel_all(INFIX | TL, panel, 2, max_hits=4) == OK
    lists = PH.all_hits(texts, panel, [2] * 4, INFIX, 0)
    before = (rb.panel_hit_counts()[0].tolist(), fields(rb.panel_hits()[1], PH.OCC_FIELDS), fields(rb.panel_tails(), T.TAIL_FIELDS), rb.scores()[0].tolist(),
              rb.counters().tolist())
    assert before[1] == Q.capped_run(lists, 4, ROOMY)[2]
    assert rb.run_panel(INFIX, other, 1, sync=False) == OK
    assert rb.run_panel_all(PREFIX | HD, other, 3, max_hits=2, sync=False) == OK
    now = (rb.panel_hit_counts()[0].tolist(), fields(rb.panel_hits()[1], PH.OCC_FIELDS), fields(rb.panel_tails(), T.TAIL_FIELDS), rb.scores()[0].tolist(),
           rb.counters().tolist())
    assert now == before and rb.panel_queue_wanted() == -1
    with pytest.raises(capi.QuickedException):
        rb.panel_heads()
    with pytest.raises(capi.QuickedException):
        rb.panel_results()
    assert rb.fetch() == OK
    check_all(rb, texts, PH.all_hits(texts, other, [3] * 3, PREFIX, 0), 2, ROOMY, None, H.all_heads(texts, other, [3] * 3, 0, 3))
    rb.close()


def test_refusals_on_the_device():
    texts, panel = small_set(10, 3, 77)
    rb = batch_of(texts, max_total=None)
    assert rb.run_panel(INFIX, panel, 2, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX, panel, 2, max_hits=4, sync=False) == capi.QUICKED_UNIMPLEMENTED
    for bad in (-1, (1 << 26) + 1):
        assert rb.configure_panel_queue(bad) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX, panel, 2, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure_panel_queue(64) == OK
    assert rb.run_panel(INFIX, panel, 2, matrix=True, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | capi.PANEL_CIGARS, panel, 2, max_hits=4, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_scan(INFIX, panel, 2, max_hits=4, window=64, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(PREFIX | TL, panel, 2, max_hits=4, sync=False) == capi.QUICKED_ERROR
    assert rb.fetch() == OK and rb.panel_queue_wanted() == -1
    assert rb.run_panel_all(INFIX, panel, 2, max_hits=4, sync=False) == OK and rb.fetch() == OK
    assert rb.panel_queue_wanted() >= 0
    assert rb.configure_panel_queue(0) == OK
    assert rb.run_panel_all(INFIX, panel, 2, max_hits=4, sync=False) == capi.QUICKED_UNIMPLEMENTED
    rb.close()


# ---- at size ------------------------------------------------------------------------------------------------------------------
def test_at_size_against_the_sync_run_and_a_sample_of_the_definition():
    """2 000 live texts x 8 members, queued, against the sync run of the same batch, with 64 texts against the definition"""
    texts, panel = small_set(2041, 8, 20261020, empty_every=50)
    assert sum(len(t) > 0 for t in texts) == 2000
    rb = batch_of(texts)
    rng = np.random.default_rng(1)
    sample = sorted(int(i) for i in rng.choice(len(texts), 64, replace=False))
    for mode, bits in ((INFIX, TL | HD), (PREFIX, 0)):
        assert rb.run_panel_all(mode | bits, panel, 3, max_hits=16) == OK
        sync = (rb.panel_hit_counts()[0].tolist(), rb.panel_hits()[0].tolist(), rb.panel_hits()[1].tobytes(), rb.scores()[0].tolist(), rb.scores()[1].tolist(),
                int(rb.counters()[0]), rb.panel_heads().tobytes() if bits else None, rb.panel_tails().tobytes() if bits else None)
        queued(rb, rb.run_panel_all, mode | bits, panel, 3, max_hits=16)
        off, hits = rb.panel_hits()
        got = (rb.panel_hit_counts()[0].tolist(), off.tolist(), hits.tobytes(), rb.scores()[0].tolist(), rb.scores()[1].tolist(),
               int(rb.counters()[0]), rb.panel_heads().tobytes() if bits else None, rb.panel_tails().tobytes() if bits else None)
        assert got == sync and rb.panel_queue_wanted() == off[-1] >= len(texts) // 4      # (PREFIX: every other text begins with a member)
        rows = fields(hits, PH.OCC_FIELDS)
        for i in sample:
            want = PH.text_hits(texts[i], panel, [3] * 8, mode, 0)
            assert rows[off[i]:off[i + 1]] == want[:16] and int(rb.panel_hit_counts()[0][i]) == len(want), i
    rb.close()
