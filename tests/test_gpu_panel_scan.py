"""Windowed panel search on the GPU (quicked_batch_run_panel_scan through capi.ResidentBatch.run_panel_scan): run_panel_all's
results, exactly, whatever the window.  Expected values never come from the library: tests/panel_hits_lib.py over the lists
recorded in tests/golden/panel_scan_cases.json (the window-boundary set) and tests/golden/panel_hits_cases.json (INFIX), or computed
live for the small sets made here, through test_gpu_panel_hits.run_and_compare itself -- the batch is handed to it behind a proxy
whose run_panel_all is the scan run at the window under test.  The one test at size compares the scan run with run_panel_all on the
same batch, array for array, and looks for what was planted."""
import numpy as np
import pytest

import panel_hits_lib as PH
import test_gpu_panel_hits as TG
from quicked_amd import capi

pytestmark = pytest.mark.gpu

INFIX = capi.SEARCH_INFIX
FLAGS = TG.FLAGS
WINDOWS = [64, 128, 0]
GS = TG._load("make_panel_scan_cases")


@pytest.fixture(scope="module")
def sets():
    out = dict(TG.G.load())
    out.update(GS.load())
    return out


class Scanned:
    """a ResidentBatch whose run_panel_all is run_panel_scan at one window: what run_and_compare is handed"""

    def __init__(self, rb, window):
        self._rb, self._window = rb, window

    def __getattr__(self, name):
        return getattr(self._rb, name)

    def run_panel_all(self, mode, panel, max_dist=None, max_hits=16, sync=True):
        return self._rb.run_panel_scan(mode, panel, max_dist, max_hits=max_hits, window=self._window, sync=sync)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("nslices", TG.SLICES)
@pytest.mark.parametrize("name", ["windows", "named", "random"])
def test_the_three_sets(sets, name, nslices, window, monkeypatch):
    s = sets[name]
    texts, panel = s["texts"], s["panel"]
    TG.slices(monkeypatch, nslices)
    rb = TG.batch_of(texts)
    for flag in FLAGS:
        for conf in ("own", "uniform"):
            want = s["hits"][(INFIX, flag, conf)]
            for cap in TG.CAPS:
                rb.kernel_times()
                TG.run_and_compare(Scanned(rb, window), texts, panel, INFIX, flag, s["bounds"] if conf == "own" else s["uniform"], cap, want)
                _, launches = rb.kernel_times()
                assert launches[0] >= (2 if any(want) else 1) and rb.counters()[0] > 0      # both passes: slot [0]
    rb.close()


@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches(sets, wire):
    """the texts of each set that the wire format can carry, packed and as ASCII: the same lists, the fixture's"""
    ok = set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN")
    for name in ("windows", "random"):
        s = sets[name]
        keep = [i for i, t in enumerate(s["texts"]) if t and set(t) <= ok]
        texts = [s["texts"][i] for i in keep]
        assert len(texts) >= 20
        patterns = [b"ACGT"] * len(texts)                  # (the wire packers take upper-case ACGT / N)
        rp, ra = TG.batch_of(texts, patterns, wire=wire), TG.batch_of(texts, patterns)
        for window in (64, 0):
            for flag in FLAGS:
                want = [s["hits"][(INFIX, flag, "own")][i] for i in keep]
                res = []
                for rb in (rp, ra):
                    assert rb.run_panel_scan(INFIX | flag, s["panel"], s["bounds"], max_hits=64, window=window) == capi.QUICKED_OK
                    res.append(TG.got_lists(rb))
                assert res[0][0].tolist() == res[1][0].tolist() and res[0][2] == res[1][2], (name, window, flag)
                assert res[0][0].tolist() == [len(h) for h in want] and res[0][2] == [h[:64] for h in want], (name, window, flag)
        rp.close()
        ra.close()


@pytest.mark.parametrize("nslots", [1, 63, 64, 65])
def test_partial_waves(nslots, monkeypatch):
    """that many window slots at a window of 64: one long text, and short texts of one window each"""
    rng = np.random.default_rng(500 + nslots)
    panel = [TG._rand(rng, int(m)) for m in (12, 20, 33, 70)]
    long_text = bytearray(TG._rand(rng, 64 * (nslots - 1) + 17))
    for at in range(30, len(long_text) - 80, 150):
        q = TG.G.mutate(rng, panel[(at // 150) % 4], 0.05)
        long_text[at:at + len(q)] = q
    shorts = [TG.G.plant(rng, int(rng.integers(20, 65)), [TG.G.mutate(rng, panel[i % 2], 0.06)])[:64] for i in range(nslots)]
    for texts in ([bytes(long_text)], shorts):
        assert sum((len(t) + 63) // 64 for t in texts) == nslots
        want = PH.all_hits(texts, panel, [4] * 4, INFIX, 0)
        rb = TG.batch_of(texts)
        for nslices in (None, "2"):
            TG.slices(monkeypatch, nslices)
            for cap in (1, 64):
                TG.run_and_compare(Scanned(rb, 64), texts, panel, INFIX, 0, 4, cap, want)
        rb.close()


def test_the_batch_patterns_play_no_part(sets):
    s = sets["windows"]
    texts, panel = s["texts"], s["panel"]
    rng = np.random.default_rng(9)
    long_patterns = [TG._rand(rng, 700 - 13 * (i % 40)) for i in range(len(texts))]
    for patterns in (None, long_patterns):
        rb = TG.batch_of(texts, patterns)
        for window in (64, 0):
            TG.run_and_compare(Scanned(rb, window), texts, panel, INFIX, 0, s["bounds"], 64, s["hits"][(INFIX, 0, "own")])
        rb.close()


def test_the_run_kinds_in_turn(sets):
    s = sets["windows"]
    texts, panel = s["texts"], s["panel"]
    patterns = [panel[i % len(panel)] for i in range(len(texts))]
    rb = TG.batch_of(texts, patterns)
    for getter in (rb.panel_hits, rb.panel_hit_counts):
        with pytest.raises(capi.QuickedException):
            getter()
    want = s["hits"][(INFIX, 0, "uniform")]
    for window in (64, 0):
        TG.run_and_compare(Scanned(rb, window), texts, panel, INFIX, 0, s["uniform"], 2, want)
        TG.run_and_compare(rb, texts, panel, INFIX, 0, s["uniform"], 2, want)                       # run_panel_all
        assert rb.run_panel(INFIX, panel, s["uniform"]) == capi.QUICKED_OK
        r = rb.panel_results()
        assert [PH.best_two(h)[:2] for h in want] == [(int(x["pattern"]), int(x["score"])) for x in r]
        for getter in (rb.panel_hits, rb.panel_hit_counts, rb.hits):
            with pytest.raises(capi.QuickedException):
                getter()
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
    s = sets["windows"]
    rb = TG.batch_of(s["texts"][:8])
    panel = s["panel"]
    assert rb.run_panel_scan(INFIX, panel, 3, window=64) == capi.QUICKED_OK
    before = TG.got_lists(rb)
    cnt = rb.counters()[0]
    for window in (-64, 1, 63, 96, 2**31 - 1):
        assert rb.run_panel_scan(INFIX, panel, 3, window=window) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | capi.SEARCH_IUPAC | capi.SEARCH_IUPAC_PATTERN, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | capi.PANEL_MATRIX, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX, panel + [b""], 3) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX, panel, -1) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX, panel, 3, max_hits=0) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX, panel, 3, max_hits=4097) == capi.QUICKED_ERROR
    for window in (0, 64):
        assert rb.run_panel_scan(capi.SEARCH_PREFIX, panel, 3, window=window) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_scan(INFIX, panel + [b"A" * 257], 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_scan(INFIX, panel, 3, sync=False) == capi.QUICKED_UNIMPLEMENTED
    after = TG.got_lists(rb)
    assert after[0].tolist() == before[0].tolist() and after[2] == before[2] and rb.counters()[0] == cnt      # nothing ran
    rb.close()


def test_long_texts_at_size():
    """2 texts of 200 kb with about 200 planted members -- a third of them ending within 2 columns of a multiple of 4096 -- and 60
    texts of 150 bases x 24 members of 18 .. 40 bases, bound 3, cap 4096: windows of the library's choice, 4096 and 64 against
    run_panel_all on the same batch, array for array, and every planted position among the occurrences"""
    rng = np.random.default_rng(2026)
    k, bound, cap, n_long = 24, 3, 4096, 200_000
    acgt = np.frombuffer(TG.ACGT, dtype=np.uint8)
    panel = [TG._rand(rng, int(rng.integers(18, 41))) for _ in range(k)]
    texts, planted = [], []
    for i in range(2):
        t = acgt[rng.integers(0, 4, n_long)].copy()
        ends = [c + int(rng.integers(-2, 3)) for c in range(4096, 4096 * 35, 4096)]              # 34 at a multiple of 4096 +- 2
        ends += [c + 2048 + int(rng.integers(-500, 501)) for c in range(0, 4096 * 48, 4096)]      # 48 in the middle of a stretch
        ends += [c + 1000 + int(rng.integers(-200, 201)) for c in range(0, 4096 * 18, 4096)]      # 18 more: 100, none overlaps another
        for end in ends:
            p = int(rng.integers(0, k))
            t[end - len(panel[p]):end] = np.frombuffer(panel[p], dtype=np.uint8)
            planted.append((i, p, end))
        texts.append(t.tobytes())
    texts += [acgt[rng.integers(0, 4, 150)].tobytes() for _ in range(60)]
    for i in range(2, 62, 3):
        p = int(rng.integers(0, k))
        at = int(rng.integers(0, 150 - len(panel[p]) + 1))
        texts[i] = texts[i][:at] + panel[p] + texts[i][at + len(panel[p]):]
        planted.append((i, p, at + len(panel[p])))
    assert sum(1 for i, _, e in planted if i < 2 and min(e % 4096, 4096 - e % 4096) <= 2) >= 60
    rb = TG.batch_of(texts)
    assert rb.run_panel_all(INFIX, panel, bound, max_hits=cap) == capi.QUICKED_OK
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    sc, st = rb.scores()
    assert np.array_equal(found, stored) and int(found[:2].min()) >= 100
    have = {(i, int(h["pattern"]), int(h["text_end"])) for i in range(len(texts)) for h in hits[off[i]:off[i + 1]] if h["score"] == 0}
    assert set(planted) <= have, sorted(set(planted) - have)[:5]
    for window in (0, 4096, 64):
        assert rb.run_panel_scan(INFIX, panel, bound, max_hits=cap, window=window) == capi.QUICKED_OK
        f2, s2 = rb.panel_hit_counts()
        o2, h2 = rb.panel_hits()
        sc2, st2 = rb.scores()
        assert np.array_equal(f2, found) and np.array_equal(s2, stored) and np.array_equal(o2, off), window
        assert np.array_equal(h2, hits), (window, int((h2 != hits).sum()))
        assert np.array_equal(sc2, sc) and np.array_equal(st2, st), window
    rb.close()
