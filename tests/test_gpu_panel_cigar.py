"""Occurrence alignments on the GPU (QUICKED_PANEL_CIGARS through capi.ResidentBatch.run_panel_all / run_panel_scan and
panel_hit_cigars): the CIGAR of every stored occurrence.  Expected strings never come from the library: they are
tests/panel_cigar_lib.py's -- the full matrix and the traceback rule in Python -- recorded in tests/golden/panel_cigar_cases.json
(a sample of which tests/test_panel_cigar_cpu.py recomputes) or computed live for the small sets made here; styles 1 and 2 go
through oracle_lib.sam_cigar.  The one test at size compares the library's two routes with each other, string for string (the
flagged panel run against (member, stretch) pairs through run_bounded with CIGARs), and a fixed sample with the definition."""
import importlib.util
import os
import re

import numpy as np
import pytest

import panel_cigar_lib as PC
import panel_hits_lib as PH
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX, CG = capi.SEARCH_PREFIX, capi.SEARCH_INFIX, capi.PANEL_CIGARS
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "4096"]
# (cap, the styles run at it): every style at the cap that stores most, one style each at the small caps
CAPS = [(1, (1,)), (2, (2,)), (64, (0, 1, 2))]
# (mode, window): -1 = run_panel_all; 64 and 0 = run_panel_scan at the smallest window and at the library's
ROUTES = [(PREFIX, -1), (INFIX, -1), (INFIX, 64), (INFIX, 0)]
ACGT = b"ACGT"


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_panel_cigar_cases")
GS = _load("make_panel_scan_cases")
WINDOWS_CAP = 4


@pytest.fixture(scope="module")
def sets():
    """the fixture's two sets, and the window-boundary set of the windowed search with the definition's strings for every text's
    first WINDOWS_CAP occurrences (INFIX, the members' own bounds)"""
    out = dict(G.load())
    w = dict(GS.load()["windows"])
    w["hits"] = {k: v for k, v in w["hits"].items() if k[2] == "own"}
    w["cigars"] = {k: [PC.hit_cigars(t, w["panel"], h[:WINDOWS_CAP], k[1]) for t, h in zip(w["texts"], v)] for k, v in w["hits"].items()}
    out["windows"] = w
    return out


def _pool(seqs):
    pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    return pool, off, ln


def batch_of(texts, patterns=None, wire=None):
    patterns = [b""] * len(texts) if patterns is None else patterns
    pp, po, pl = _pool(patterns)
    tp, to, tl = _pool(texts)
    return capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl), wire=wire)


def env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def run(rb, mode, panel, bounds, cap, window):
    arg = bounds if np.ndim(bounds) == 0 else np.asarray(bounds, dtype=np.int32)
    if window < 0:
        return rb.run_panel_all(mode, panel, arg, max_hits=cap)
    return rb.run_panel_scan(mode, panel, arg, max_hits=cap, window=window)


def records(rb):
    """-> (found, off, [(pattern, text_start, text_end, score)], scores, statuses, counter [0])"""
    found, stored = rb.panel_hit_counts()
    off, hits = rb.panel_hits()
    rows = np.stack([hits[f] for f in PH.OCC_FIELDS], axis=1).astype(np.int64).tolist() if len(hits) else []
    sc, st = rb.scores()
    return found.tolist(), off.tolist(), [tuple(r) for r in rows], sc.tolist(), st.tolist(), int(rb.counters()[0])


def flagged_and_plain(rb, mode, panel, bounds, cap, window):
    """the run without the bit, then with it: -> (the flagged run's records, its strings); everything the first leaves is left
    unchanged, counter [0] included, and the strings exist after the second only"""
    assert run(rb, mode, panel, bounds, cap, window) == capi.QUICKED_OK
    plain = records(rb)
    with pytest.raises(capi.QuickedException):
        rb.panel_hit_cigars()
    assert rb.counters()[1] == 0 and rb.counters()[3] == 0
    rb.kernel_times()
    assert run(rb, mode | CG, panel, bounds, cap, window) == capi.QUICKED_OK
    got = records(rb)
    assert got == plain
    cig = rb.panel_hit_cigars()
    assert len(cig) == got[1][-1] and all(c for c in cig)
    assert all(c is None for c in rb.cigars())                         # quicked_batch_cigars: -1 for every pair
    for getter in (rb.locations, rb.hits, rb.panel_results, rb.panel_matrix):
        with pytest.raises(capi.QuickedException):
            getter()
    return got, cig


def check_strings(s, key, cap, style, got, cig, panel, prefix):
    """every stored occurrence's record and string against the recorded ones; the invariants; counters [1] and [3] are checked by
    the caller from what this returns: (block steps, operations) of the stored occurrences"""
    want_h, want_c = s["hits"][key], s["cigars"][key]
    found, off, rows = got[0], got[1], got[2]
    steps = ops = 0
    for i, (h, cs) in enumerate(zip(want_h, want_c)):
        keep = min(len(h), cap)
        assert found[i] == len(h) and off[i + 1] - off[i] == keep, (key, cap, i)
        for k in range(min(keep, len(cs))):                            # (a set may carry strings for a text's first few only)
            j = off[i] + k
            assert rows[j] == h[k], (key, cap, i, k)
            want = PC.styled(cs[k], style)
            assert cig[j] == want, (key, cap, style, i, k, rows[j], cig[j], want)
        for k in range(keep):
            p, a, e, v = rows[off[i] + k]
            PC.invariants(cig[off[i] + k], style, len(panel[p]), e - a, v, prefix)
            steps += ((len(panel[p]) + 63) // 64) * (e - a)
            ops += sum(int(x) for x in re.findall(r"(\d+)", cig[off[i] + k]))
    return steps, ops


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name", ["named", "random", "windows"])
def test_the_sets(sets, name, nslices, monkeypatch):
    s = sets[name]
    texts, panel = s["texts"], s["panel"]
    env(monkeypatch, "QE_PANEL_SLICES", nslices)
    rb = batch_of(texts)
    for mode, window in ROUTES:
        for flag in FLAGS:
            for conf in ("own", "uniform"):
                key = (mode, flag, conf)
                if key not in s["cigars"]:
                    continue
                bounds = s["bounds"] if conf == "own" else s["uniform"]
                for cap, styles in CAPS:
                    for style in styles:
                        assert rb.configure(style) == capi.QUICKED_OK
                        got, cig = flagged_and_plain(rb, mode | flag, panel, bounds, cap, window)
                        steps, ops = check_strings(s, key, cap, style, got, cig, panel, mode == PREFIX)
                        c = rb.counters()
                        assert c[1] == steps and c[3] == ops, (key, cap, style, c[:4].tolist(), steps, ops)
                        _, launches = rb.kernel_times()
                        assert launches[1] == (1 if cig else 0) and launches[0] >= 1
    rb.close()


def one_hit_texts(n, seed):
    """n texts with exactly one occurrence of the one member within bound 1 each: n stored occurrences at cap 1"""
    rng = np.random.default_rng(seed)
    member = b"ACGTTGCAAGGCTTAACCGT"
    texts = []
    for i in range(n):
        q = bytearray(member)
        if i % 3 == 1:
            q[7] = ord("A") if q[7] != ord("A") else ord("C")
        elif i % 3 == 2:
            del q[11]
        texts.append(bytes(rng.choice(np.frombuffer(b"CT", dtype=np.uint8), 9 + i % 5)) + bytes(q) + bytes(rng.choice(np.frombuffer(b"CT", dtype=np.uint8), 6)))
    return texts, [member]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_partial_waves(n):
    texts, panel = one_hit_texts(n, 40 + n)
    want = PH.all_hits(texts, panel, [1], INFIX, 0)
    assert all(len(h) == 1 for h in want)
    s = {"hits": {0: want}, "cigars": {0: [PC.hit_cigars(t, panel, h, 0) for t, h in zip(texts, want)]}}
    rb = batch_of(texts)
    for window in (-1, 64):
        got, cig = flagged_and_plain(rb, INFIX, panel, 1, 1, window)
        assert len(cig) == n
        check_strings(s, 0, 1, 0, got, cig, panel, False)
    rb.close()


def test_many_launches_under_a_small_history_budget(sets, monkeypatch):
    """QE_PANEL_ALIGN_WS_KB = 1: one wave of occurrences per launch, all of them sharing one history"""
    s = sets["named"]
    texts, panel = s["texts"], s["panel"]
    rb = batch_of(texts)
    env(monkeypatch, "QE_PANEL_ALIGN_WS_KB", "1")
    for mode, window in ROUTES:
        key = (mode, capi.SEARCH_IUPAC, "own")
        got, cig = flagged_and_plain(rb, mode | capi.SEARCH_IUPAC, panel, s["bounds"], 64, window)
        check_strings(s, key, 64, 0, got, cig, panel, mode == PREFIX)
        _, launches = rb.kernel_times()
        assert len(cig) > 64 and launches[1] == (len(cig) + 63) // 64 > 1, (len(cig), launches.tolist())
    rb.close()


@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches(sets, wire):
    s = sets["random"]
    ok = set(b"ACGT") if wire == capi.WIRE_2BIT else set(b"ACGTN")
    keep = [i for i, t in enumerate(s["texts"]) if t and set(t) <= ok]
    texts = [s["texts"][i] for i in keep]
    assert len(texts) >= 20
    rb = batch_of(texts, [b"ACGT"] * len(texts), wire=wire)
    for mode, window in ROUTES:
        for flag in FLAGS:
            key = (mode, flag, "own")
            sub = {"hits": {key: [s["hits"][key][i] for i in keep]}, "cigars": {key: [s["cigars"][key][i] for i in keep]}}
            got, cig = flagged_and_plain(rb, mode | flag, s["panel"], s["bounds"], 64, window)
            check_strings(sub, key, 64, 0, got, cig, s["panel"], mode == PREFIX)
    rb.close()


def test_argument_rules_on_the_device(sets):
    s = sets["named"]
    rb = batch_of(s["texts"][:8])
    panel = s["panel"]
    with pytest.raises(capi.QuickedException):
        rb.panel_hit_cigars()
    assert rb.run_panel_all(INFIX | CG, panel, 3) == capi.QUICKED_OK
    before, cig, cnt = records(rb), rb.panel_hit_cigars(), rb.counters().tolist()
    assert rb.run_panel(INFIX | CG, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | CG | capi.PANEL_MATRIX, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(INFIX | CG | capi.PANEL_MATRIX, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_all(INFIX | CG | 128, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel_scan(PREFIX | CG, panel, 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | CG, panel, 3, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel_all(INFIX | CG, panel + [b"A" * 257], 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(0, True) == capi.QUICKED_OK
    assert rb.run_panel_all(INFIX | CG, panel, 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(0, False) == capi.QUICKED_OK
    assert records(rb) == before and rb.panel_hit_cigars() == cig and rb.counters().tolist() == cnt      # nothing ran
    assert rb.run_panel(INFIX, panel, 3) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.panel_hit_cigars()
    rb.close()


def _rand(rng, n):
    return bytes(ACGT[int(x)] for x in rng.integers(0, 4, n))


def test_route_agreement_at_size():
    """2 000 texts of 150 bases x 24 members of 24, INFIX, bound 4: every stored occurrence's string is the pair route's --
    (member, stretch) through run_bounded with bound = score and CIGARs, in the same style -- and a fixed sample of 200 is the
    definition's"""
    rng = np.random.default_rng(79)
    n, k, cap, bound = 2000, 24, 6, 4
    panel = [_rand(rng, 24) for _ in range(k)]
    codes = rng.integers(0, 4, (n, 150)).astype(np.uint8)
    tarr = np.frombuffer(ACGT, dtype=np.uint8)[codes]
    for i in range(n):
        at = 0
        for _ in range(i % 4):                                         # 0 .. 3 members per text, with a few errors each
            q = bytearray(panel[int(rng.integers(0, k))])
            for _ in range(int(rng.integers(0, 4))):
                pos, how = int(rng.integers(0, len(q))), int(rng.integers(0, 3))
                if how == 0:
                    q[pos] = ACGT[int(rng.integers(0, 4))]
                elif how == 1:
                    del q[pos]
                else:
                    q.insert(pos, ACGT[int(rng.integers(0, 4))])
            if at + len(q) > 150:
                break
            at = int(rng.integers(at, 150 - len(q) + 1))
            tarr[i, at:at + len(q)] = np.frombuffer(bytes(q), dtype=np.uint8)
            at += len(q)
    texts = [tarr[i].tobytes() for i in range(n)]
    rb = batch_of(texts)
    for style in (0, 2):
        assert rb.configure(style) == capi.QUICKED_OK
        got, cig = flagged_and_plain(rb, INFIX, panel, bound, cap, -1)
        found, off, rows = got[0], got[1], got[2]
        assert len(rows) > n // 2 and max(r[3] for r in rows) <= bound and {0, 1, 2} <= {r[3] for r in rows}
        text_of = np.repeat(np.arange(n), np.diff(off))
        members = [panel[r[0]] for r in rows]
        stretches = [texts[int(i)][r[1]:r[2]] for i, r in zip(text_of, rows)]
        pp, po, pl = _pool(members)
        tp, to, tl = _pool(stretches)
        rq = capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl))
        assert rq.configure(style) == capi.QUICKED_OK
        assert rq.run_bounded(np.array([r[3] for r in rows], dtype=np.int32), only_score=False) >= 0
        sc, _ = rq.scores()
        pair_cig = rq.cigars()
        rq.close()
        assert sc.tolist() == [r[3] for r in rows]
        bad = [j for j in range(len(rows)) if cig[j] != pair_cig[j]]
        assert not bad, (style, len(bad), [(rows[j], cig[j], pair_cig[j]) for j in bad[:4]])
        sample = [int(j) for j in np.random.default_rng(5).choice(len(rows), 200, replace=False)]
        for j in sample:
            d, c = PC.cigar(members[j], stretches[j], 0)
            assert d == rows[j][3] and cig[j] == PC.styled(c, style), (style, j, rows[j], cig[j], c)
            PC.invariants(cig[j], style, 24, rows[j][2] - rows[j][1], rows[j][3])
    rb.close()
