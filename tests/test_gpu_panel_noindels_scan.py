"""The windowed mismatch-only panel run on the GPU (quicked_batch_run_panel_scan_no_indels through
capi.ResidentBatch.run_panel_scan_no_indels): the flagged run_panel_all's results, exactly, whatever the window.  Expected values
never come from the library: tests/panel_noindels_lib.py's lists as recorded in tests/golden/panel_noindels_scan_cases.json (the
window-boundary set, with the block steps of tests/panel_noindels_scan_lib.py's rule) and tests/golden/panel_noindels_cases.json
(its INFIX cases), or computed live for the small sets made here.  Every run is also compared with run_panel_all(mode |
PANEL_NO_INDELS) on the same batch, array for array; the one test at size has that comparison and what was planted."""
import numpy as np
import pytest

import panel_noindels_lib as N
import panel_noindels_scan_lib as S
import test_gpu_panel_noindels as TN
from quicked_amd import capi

pytestmark = pytest.mark.gpu

INFIX, NI = capi.SEARCH_INFIX, capi.PANEL_NO_INDELS
FLAGS = TN.FLAGS
WINDOWS = [64, 128, 0]
CAPS = (1, 2, 16)
GS = TN._load("make_panel_noindels_scan_cases")
BOUNDARY = GS.load()
UNWINDOWED_STEPS = GS.load_unwindowed_steps()      # {group of panel_noindels_cases.json: {flag: [steps at S.NATIVE_WINDOWS]}}


def plain(g):
    return not any(set(s.upper()) - set(b"ACGT") for s in g["texts"] + g["panel"])


def lists_of(g, flag):
    """the uncapped lists of a boundary group under a flag: recorded, or -- upper and lower case ACGT alone, where the three
    equalities agree -- the unflagged record"""
    if flag in g["results"]:
        return g["results"][flag]
    assert plain(g), g["name"]
    return g["results"][0]


def steps_of(recorded, flag, window, texts, panel):
    """the model's block steps of a run: recorded per flag at the forced windows; at window 0 every text of these sets is one
    slot -- the library's choice is min(the longest text rounded up to 64, 1024) columns for batches this small -- and one
    slot per text walks every start once"""
    if window == 0:
        assert max(len(t) for t in texts) <= 1024
        return N.block_steps(texts, panel, INFIX)
    return (recorded[flag] if flag in recorded else recorded[0])[S.NATIVE_WINDOWS.index(window)]


def arrays_of(rb):
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    sc, st = rb.scores()
    return found, stored, off, hits, sc, st


def same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def scan_and_compare(rb, texts, panel, bounds, flag, cap, window, want, steps, bit=NI):
    """the flagged run_panel_all, then the scan at `window`: array-identical, the lists' first `cap` (want: per text at least its
    first `cap` occurrences, or None), counter [0] = steps, the model's, [1] .. [7] = 0, one timed launch"""
    md = np.asarray(bounds, dtype=np.int32)
    assert rb.run_panel_all(INFIX | flag | NI, panel, md, max_hits=cap) == capi.QUICKED_OK
    A = arrays_of(rb)
    rb.kernel_times()
    assert rb.run_panel_scan_no_indels(INFIX | flag | bit, panel, md, max_hits=cap, window=window) == capi.QUICKED_OK
    R = arrays_of(rb)
    assert same_arrays(A, R), (flag, cap, window, [i for i in range(len(texts)) if A[0][i] != R[0][i]][:5])
    found, stored, got = TN.got_lists(rb)
    if want is not None:
        bad = [(i, int(found[i]), got[i][:3], want[i][:3]) for i in range(len(texts)) if got[i] != [tuple(o) for o in want[i][:cap]] or int(found[i]) < len(got[i])]
        assert not bad, (flag, cap, window, len(bad), bad[:4])
        assert stored.tolist() == [min(int(f), cap) for f in found]
    assert R[5].tolist() == [capi.QUICKED_OK if t else capi.QUICKED_EMPTY_SEQUENCE for t in texts]
    counters = rb.counters()
    assert int(counters[0]) == steps and not any(int(c) for c in counters[1:]), (flag, cap, window, counters, steps)
    _, launches = rb.kernel_times()
    assert launches[0] == 1 and not any(launches[1:])                      # the sweep alone: no start pass
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix, rb.panel_hit_cigars, rb.panel_tails, rb.panel_heads):
        with pytest.raises(capi.QuickedException):
            getter()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("nslices", TN.SLICES)
def test_the_boundary_set(nslices, window, monkeypatch):
    TN.slices(monkeypatch, nslices)
    for g in BOUNDARY:
        texts, panel, bounds = g["texts"], g["panel"], g["bounds"]
        rb = TN.batch_of(texts)
        for flag in FLAGS:
            want = lists_of(g, flag)
            steps = steps_of(g["steps"], flag, window, texts, panel)
            for cap in CAPS:
                scan_and_compare(rb, texts, panel, bounds, flag, cap, window, want, steps, bit=NI if cap != 2 else 0)
                assert rb.panel_hit_counts()[0].tolist() == [len(h) for h in want]
        rb.close()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("nslices", TN.SLICES)
def test_the_unwindowed_fixture(nslices, window, monkeypatch):
    """panel_noindels_cases.json's INFIX cases (its record keeps a text's first 8 occurrences)"""
    TN.slices(monkeypatch, nslices)
    for name in TN.GROUPS:
        g = TN._RECORD[name]
        texts, panel, bounds = g["texts"], g["panel"], g["bounds"]
        rb = TN.batch_of(texts)
        for flag in FLAGS:
            r = g["results"][(INFIX, flag)]
            steps = steps_of(UNWINDOWED_STEPS[name], flag, window, texts, panel)
            for cap in CAPS:
                scan_and_compare(rb, texts, panel, bounds, flag, cap, window, r["occ"] if cap <= TN.G.CAP else None, steps)
                found, _ = rb.panel_hit_counts()
                assert found.tolist() == r["found"]
        rb.close()


@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches(wire):
    """the texts of the boundary groups that the wire format can carry, packed: the same lists"""
    seen = 0
    for g in BOUNDARY:
        keep = TN.fitting(g["texts"], wire)
        if len(keep) < 2:
            continue
        texts = [g["texts"][i] for i in keep]
        assert plain(g)                                   # (so R, and with it the steps, are the same under the three flags)
        rb = TN.batch_of(texts, wire)
        for window in (64, 0):
            steps = S.block_steps(texts, g["panel"], g["bounds"], 0, window)
            for flag in FLAGS:
                want = [lists_of(g, flag)[i] for i in keep]
                scan_and_compare(rb, texts, g["panel"], g["bounds"], flag, 16, window, want, steps)
                seen += sum(len(h) for h in want)
        rb.close()
    assert seen > 1000


@pytest.mark.parametrize("nslots", [1, 63, 64, 65])
def test_partial_waves(nslots, monkeypatch):
    """that many window slots at a window of 64: one long text, and short texts of one window each"""
    rng = np.random.default_rng(700 + nslots)
    panel = [TN._rand(rng, int(m)) for m in (12, 20, 33, 70)]
    bounds = [2] * 4
    long_text = bytearray(TN._rand(rng, 64 * (nslots - 1) + 17))
    for at in range(30, len(long_text) - 80, 150):
        q = TN.G.substitute(rng, panel[(at // 150) % 4], int(rng.integers(0, 3)))
        long_text[at:at + len(q)] = q
    shorts = [TN.G.plant(rng, int(rng.integers(20, 65)), TN.G.substitute(rng, panel[i % 2], i % 3)) for i in range(nslots)]
    for texts in ([bytes(long_text)], shorts):
        assert sum((len(t) + 63) // 64 for t in texts) == nslots
        want = [N.text_hits(t, panel, bounds, INFIX, 0) for t in texts]
        steps = S.block_steps(texts, panel, bounds, 0, 64)
        rb = TN.batch_of(texts)
        for nslices in (None, "2"):
            TN.slices(monkeypatch, nslices)
            for cap in (1, 64):
                scan_and_compare(rb, texts, panel, bounds, 0, cap, 64, want, steps)
        rb.close()


def test_the_run_kinds_in_turn():
    """flagged scan, unflagged scan, flagged run_panel_all, the flagged scan again, on one batch object"""
    g = next(g for g in BOUNDARY if g["name"] == "bounds")
    texts, panel = g["texts"], g["panel"]
    md = np.asarray(g["bounds"], dtype=np.int32)
    rb = TN.batch_of(texts)
    for getter in (rb.panel_hits, rb.panel_hit_counts):
        with pytest.raises(capi.QuickedException):
            getter()
    want = [[tuple(o) for o in h[:16]] for h in g["results"][0]]
    for window in (64, 0):
        assert rb.run_panel_scan_no_indels(INFIX, panel, md, window=window) == capi.QUICKED_OK
        first = arrays_of(rb)
        assert TN.got_lists(rb)[2] == want
        assert rb.run_panel_scan(INFIX, panel, md, window=window) == capi.QUICKED_OK              # by edits: other sites, other scores
        edits = arrays_of(rb)
        assert not same_arrays(first, edits)
        assert rb.run_panel_all(INFIX | NI, panel, md) == capi.QUICKED_OK
        assert same_arrays(first, arrays_of(rb))
        assert rb.run_panel_scan_no_indels(INFIX | NI, panel, md, window=window) == capi.QUICKED_OK
        assert same_arrays(first, arrays_of(rb)) and not any(int(c) for c in rb.counters()[1:])
        assert rb.run_panel(INFIX | NI, panel, md) == capi.QUICKED_OK
        for getter in (rb.panel_hits, rb.panel_hit_counts, rb.hits):
            with pytest.raises(capi.QuickedException):
                getter()
    rb.close()


def test_refusals_on_the_device():
    g = next(g for g in BOUNDARY if g["name"] == "bytes")
    panel = g["panel"]
    rb = TN.batch_of(g["texts"])
    scan = rb.run_panel_scan_no_indels
    assert scan(INFIX | capi.SEARCH_IUPAC, panel, 1, window=64) == capi.QUICKED_OK
    before, cnt = TN.got_lists(rb), rb.counters()[0]
    assert sum(before[0]) > 0
    CG, TL, HD, MX = capi.PANEL_CIGARS, capi.PANEL_TAILS, capi.PANEL_HEADS, capi.PANEL_MATRIX
    for ni in (0, NI):
        for window in (-64, 1, 63, 96, 2**31 - 1):
            assert scan(INFIX | ni, panel, 1, window=window) == capi.QUICKED_ERROR
            assert scan(capi.SEARCH_PREFIX | ni | CG, panel, 1, window=window, sync=False) == capi.QUICKED_ERROR
        for extra in (4, 8, 128, 256, 1024, 4096, 16384, 65536, MX, TL, HD, TL | CG, capi.SEARCH_IUPAC | capi.SEARCH_IUPAC_PATTERN):
            assert scan(INFIX | ni | extra, panel, 1) == capi.QUICKED_ERROR
        assert scan(ni, panel, 1) == capi.QUICKED_ERROR and scan(3 | ni, panel, 1) == capi.QUICKED_ERROR
        assert scan(INFIX | ni, panel + [b""], 1) == capi.QUICKED_ERROR
        assert scan(INFIX | ni, panel, -1) == capi.QUICKED_ERROR
        assert scan(INFIX | ni, panel, 1, max_hits=0) == capi.QUICKED_ERROR
        assert scan(INFIX | ni, panel, 1, max_hits=4097, sync=False) == capi.QUICKED_ERROR
        for window in (0, 64):
            assert scan(capi.SEARCH_PREFIX | ni, panel, 1, window=window) == capi.QUICKED_UNIMPLEMENTED
        assert scan(INFIX | ni | CG, panel, 1) == capi.QUICKED_UNIMPLEMENTED
        assert scan(INFIX | ni, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
        assert scan(INFIX | ni, panel + [b"A" * 257], 1) == capi.QUICKED_UNIMPLEMENTED
    rb.configure_panel_queue(1 << 16)                                 # ... also on a batch object whose queue is switched on
    assert scan(INFIX | NI, panel, 1, sync=False) == capi.QUICKED_UNIMPLEMENTED
    rb.configure_panel_queue(0)
    rb.configure(check=1)
    assert scan(INFIX | NI, panel, 1) == capi.QUICKED_UNIMPLEMENTED
    rb.configure(check=0)
    assert rb.run_panel_scan(INFIX | NI, panel, 1) == capi.QUICKED_ERROR      # the bit on the edit-distance scan stays an unknown bit
    after = TN.got_lists(rb)
    assert after[0].tolist() == before[0].tolist() and after[2] == before[2] and rb.counters()[0] == cnt      # nothing ran
    rb.close()


def test_long_texts_at_size():
    """2 texts of 200 kb with 220 planted members carrying 0 .. 2 substitutions -- a third of them ending within 2 columns of a
    multiple of 4096 -- and 60 texts of 150 bases x 40 members of 20 .. 70 bases, bound 2, cap 4096: windows of the library's
    choice, 4096 and 64 against the flagged run_panel_all on the same batch, array for array, and every planted position among
    the occurrences"""
    rng = np.random.default_rng(2027)
    k, bound, cap, n_long = 40, 2, 4096, 200_000
    acgt = np.frombuffer(TN.ACGT, dtype=np.uint8)
    panel = [TN._rand(rng, int(rng.integers(20, 71))) for _ in range(k)]
    texts, planted = [], []
    for i in range(2):
        t = acgt[rng.integers(0, 4, n_long)].copy()
        ends = [c + int(rng.integers(-2, 3)) for c in range(4096, 4096 * 38, 4096)]              # 37 at a multiple of 4096 +- 2
        ends += [c + 2048 + int(rng.integers(-500, 501)) for c in range(0, 4096 * 48, 4096)]      # 48 in the middle of a stretch
        ends += [c + 1000 + int(rng.integers(-200, 201)) for c in range(0, 4096 * 15, 4096)]      # 15 more: 100, none overlaps another
        for end in ends:
            p = int(rng.integers(0, k))
            subs = int(rng.integers(0, 3))
            t[end - len(panel[p]):end] = np.frombuffer(TN.G.substitute(rng, panel[p], subs), dtype=np.uint8)
            planted.append((i, p, end, subs))
        texts.append(t.tobytes())
    texts += [acgt[rng.integers(0, 4, 150)].tobytes() for _ in range(60)]
    for i in range(2, 62, 3):
        p = int(rng.integers(0, k))
        at = int(rng.integers(0, 150 - len(panel[p]) + 1))
        subs = int(rng.integers(0, 3))
        texts[i] = texts[i][:at] + TN.G.substitute(rng, panel[p], subs) + texts[i][at + len(panel[p]):]
        planted.append((i, p, at + len(panel[p]), subs))
    assert len(planted) == 220 and 3 * sum(1 for i, _, e, _ in planted if i < 2 and min(e % 4096, 4096 - e % 4096) <= 2) >= len(planted)
    rb = TN.batch_of(texts)
    assert rb.run_panel_all(INFIX | NI, panel, bound, max_hits=cap) == capi.QUICKED_OK
    A = arrays_of(rb)
    found, stored, off, hits = A[:4]
    assert np.array_equal(found, stored) and int(found[:2].min()) >= 100
    have = {(i, int(h["pattern"]), int(h["text_end"]), int(h["score"])) for i in range(len(texts)) for h in hits[off[i]:off[i + 1]]}
    assert set(planted) <= have, sorted(set(planted) - have)[:5]
    assert all(int(h["text_start"]) == int(h["text_end"]) - len(panel[int(h["pattern"])]) for h in hits)
    whole = int(rb.counters()[0])
    for window in (0, 4096, 64):
        assert rb.run_panel_scan_no_indels(INFIX, panel, bound, max_hits=cap, window=window) == capi.QUICKED_OK
        R = arrays_of(rb)
        assert same_arrays(A, R), (window, int((R[3] != hits).sum()) if len(R[3]) == len(hits) else (len(R[3]), len(hits)))
        counters = rb.counters()
        assert int(counters[0]) >= whole and not any(int(c) for c in counters[1:]), (window, counters)
    rb.close()
