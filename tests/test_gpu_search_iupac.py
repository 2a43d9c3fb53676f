"""IUPAC degenerate-base search on the GPU (QUICKED_SEARCH_IUPAC / QUICKED_SEARCH_IUPAC_PATTERN OR-ed into the mode of
quicked_batch_run_search and quicked_batch_run_search_all, through capi.ResidentBatch).  Expected values never come from the
library: the brute-force DP of tests/iupac_lib.py (the definition, computed live and shared between the tests) and, where it
judges, edlib's recorded answers (tests/golden/search_iupac_cases.json).  Every test runs in both kernel forms through
QE_SEARCH_FORM."""
import importlib.util
import os

import numpy as np
import pytest

import iupac_lib as I
import search_lib as S
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = capi.SEARCH_PREFIX, capi.SEARCH_INFIX
IUPAC, IUPAC_PATTERN = capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN
MODES = [PREFIX, INFIX]
FLAGS = [IUPAC, IUPAC_PATTERN]
FORMS = ["0", "1"]                               # QE_SEARCH_FORM: the workspace form always / the register form where it applies
INT_MAX = 2**31 - 1
PACK_LENS = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4097)


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_iupac_cases", os.path.join(ROOT, "tests", "golden", "make_search_iupac_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _cases()
M = G.M


def _pools(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs) or b"\0", dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1])]).astype(np.int64)
    return pp, po, pl, tp, to, tl


def batch_of(pairs, wire=None):
    return capi.ResidentBatch(datagen.PairBatch(*_pools(pairs)), wire=wire)


def results(rb):
    sc, st = rb.scores()
    ts, te = rb.locations()
    return list(zip(sc.tolist(), ts.tolist(), te.tolist())), st


def expect(pairs, mode, flag, bounds):
    return [(-1, -1, -1) if not p or not t else tuple(I.bounded(I.locate(p, t, mode, flag), len(p), bd)) for (p, t), bd in zip(pairs, bounds)]


def run_and_compare(rb, pairs, mode, flag, bounds, sync=True):
    """bounds: None, one int, or one per pair"""
    if bounds is None:
        per_pair = [INT_MAX] * len(pairs)
    elif np.ndim(bounds) == 0:
        per_pair = [int(bounds)] * len(pairs)
    else:
        per_pair = [int(b) for b in bounds]
    exp = expect(pairs, mode, flag, per_pair)
    arg = bounds if (bounds is None or np.ndim(bounds) == 0) else np.asarray(bounds, dtype=np.int32)
    assert rb.run_search(mode | flag, arg, only_score=True, sync=sync) == capi.QUICKED_OK
    if not sync:
        assert rb.fetch() == capi.QUICKED_OK
    got, status = results(rb)
    bad = [(i, len(pairs[i][0]), len(pairs[i][1]), per_pair[i], got[i], exp[i]) for i in range(len(pairs)) if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:8])
    assert status.tolist() == [capi.QUICKED_OK if p and t else capi.QUICKED_EMPTY_SEQUENCE for p, t in pairs]
    assert all(c is None for c in rb.cigars())
    return exp


def cycle_bounds(pairs, mode, flag):
    """0, 1, d - 1, d, d + 1, 12, 63 and m in turn"""
    out = []
    for i, (p, t) in enumerate(pairs):
        d = I.locate(p, t, mode, flag)[0]
        out.append((0, 1, max(0, d - 1), d, d + 1, 12, 63, len(p))[i % 8])
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("flag", FLAGS)
def test_grid_named_and_random_sets(flag, form, monkeypatch):
    sets = [("grid", G.grid_cases()), ("named", G.named_cases()), ("random", G.random_cases())]
    pairs = [c for _, s in sets for c in s]
    rec = [r for name, _ in sets for r in G.expected(name)]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        rb.kernel_times()
        exp = run_and_compare(rb, pairs, mode, flag, None)
        _, launches = rb.kernel_times()
        assert launches[0] >= (2 if mode == INFIX else 1) and rb.counters()[0] > 0      # the search passes: slot [0] of both
        # edlib's record where it judges (d == m: its end location is -1, the rule of the header is the definition)
        judged = 0
        for (p, t), r, e in zip(pairs, rec, exp):
            if r is None or not I.edlib_judges(p, t, flag):
                continue
            ed = r[0 if mode == PREFIX else 1]
            assert e[0] == ed[0]
            if ed[0] != len(p):
                assert list(e) == ed, (len(p), len(t), e, ed)
                judged += 1
        assert judged >= (len(pairs) // 2 if flag == IUPAC else 1)
        run_and_compare(rb, pairs, mode, flag, 12)
        exp = run_and_compare(rb, pairs, mode, flag, cycle_bounds(pairs, mode, flag))
        assert any(e[0] < 0 for e in exp) and any(e[0] >= 0 for e in exp)
    rb.close()


def pack_boundary_pairs():
    """per length L: pattern == text over the 15 letters in mixed case, one byte outside the alphabet at position 0 / at
    position L - 1; and a pattern of L letters inside a text of L + 7 at the odd offset 5, so that the two sequences are packed
    at different alignments and a defect that treated both alike (bases permuted within or between 1024-base spans, forward
    or reversed) changes the answer"""
    rng = np.random.default_rng(G.SEED + 7)
    letters = list(b"ACGTRYSWKMBDHVNacgtryswkmbdhvn")
    out = []
    for L in PACK_LENS:
        for at in (0, L - 1):
            s = bytearray(M._rand(rng, L, letters))
            s[at] = ord("-") if at == 0 else ord("*")
            out.append((bytes(s), bytes(s)))
        s = bytes(M._rand(rng, L, letters))
        out.append((s, bytes(M._rand(rng, 5, letters)) + s + bytes(M._rand(rng, 2, letters))))
    return out


@pytest.mark.parametrize("form", FORMS)
def test_pack_boundaries(form, monkeypatch):
    pairs = pack_boundary_pairs()
    assert sorted({len(p) for p, _ in pairs}) == list(PACK_LENS)
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for flag in FLAGS:
        for mode in MODES:                          # INFIX reads the reversed pack in its start pass
            exp = run_and_compare(rb, pairs, mode, flag, None)
            if flag == IUPAC:                       # the byte outside the alphabet equals nothing, itself included: one edit (L = 1: d = m)
                assert all(e[0] == 1 for (p, t), e in zip(pairs, exp) if p == t)
                if mode == INFIX:                   # the planted copy is found where it lies (or, degenerate letters allowing, earlier)
                    assert all(e[0] == 0 and e[2] <= 5 + len(p) for (p, t), e in zip(pairs, exp) if p != t)
                    assert sum(1 for (p, t), e in zip(pairs, exp) if p != t and e[1:] == (5, 5 + len(p))) >= len(PACK_LENS) - 3
    rb.close()


def hits_of(rb):
    found, off, hits = rb.hits()
    return found.tolist(), [[(int(h["text_start"]), int(h["text_end"]), int(h["score"])) for h in hits[off[i]:off[i + 1]]] for i in range(len(found))]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("flag", FLAGS)
def test_all_occurrences(flag, form, monkeypatch):
    pairs = G.tie_cases() + G.named_cases() + G.random_cases()[:200]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    multi = 0
    for mode in MODES:
        for bound in (2, 12):
            occ = [I.occurrences(p, t, mode, flag, bound) for p, t in pairs]
            multi += sum(1 for o in occ if len(o) > 1)
            for cap in (1, 2, 16):
                assert rb.run_search_all(mode | flag, bound, max_hits=cap) == capi.QUICKED_OK
                found, hits = hits_of(rb)
                assert found == [len(o) for o in occ]
                bad = [(i, hits[i], occ[i][:cap]) for i in range(len(pairs)) if hits[i] != occ[i][:cap]]
                assert not bad, (len(bad), bad[:6])
                sc, _ = rb.scores()
                assert sc.tolist() == [min((x[2] for x in o), default=-1) for o in occ]
            # the best occurrence is the flagged best search's answer at the same bound
            assert rb.run_search(mode | flag, bound) == capi.QUICKED_OK
            best = results(rb)[0]
            for i, o in enumerate(occ):
                want = (-1, -1, -1)
                if o:
                    d = min(x[2] for x in o)
                    s, e, _ = next(x for x in o if x[2] == d)
                    want = (d, s, e)
                assert best[i] == want, (i, best[i], want)
    assert multi > 20
    rb.close()


def _degenerate_patterns(pairs, seed):
    """a seeded 2 % of the pattern bases replaced by a random IUPAC letter that contains the base"""
    rng = np.random.default_rng(seed)
    out = []
    for p, t in pairs:
        q = bytearray(p)
        for pos in np.nonzero(rng.random(len(q)) < 0.02)[0]:
            c = G.CONTAINING[q[pos]]
            q[pos] = ord(c[int(rng.integers(0, len(c)))])
        out.append((bytes(q), t))
    return out


def _with_form(form, fn):
    os.environ["QE_SEARCH_FORM"] = form
    capi.reload_env()
    try:
        return fn()
    finally:
        del os.environ["QE_SEARCH_FORM"]
        capi.reload_env()


def test_acgt_invariant_at_size():
    """20 000 pairs of a 150-base pattern in a 400-base text at 4 %: on ACGT input a flagged run equals the unflagged one for
    every pair, in both forms; with 2 % of the pattern bases made degenerate the brute force judges a seeded sample of 200,
    and no score is larger than the unflagged score of the original pair"""
    pairs = M.big_batch()
    assert len(pairs) == M.BIG["count"]
    bound = M.BIG["bound"]
    sample = M.big_sample_indices()
    rb = batch_of(pairs)

    def run(b, mode, bd):
        assert b.run_search(mode, bd) == capi.QUICKED_OK
        return results(b)[0]

    plain = {}
    for mode in MODES:
        for form in FORMS:
            plain[mode] = _with_form(form, lambda: run(rb, mode, bound))
            for flag in FLAGS:
                assert _with_form(form, lambda: run(rb, mode | flag, bound)) == plain[mode], (mode, flag, form)
    unbounded = run(rb, INFIX, None)
    rb.close()
    deg = _degenerate_patterns(pairs, G.SEED + 8)
    assert sum(1 for (p, _), (q, _) in zip(pairs, deg) if p != q) > len(pairs) // 2
    rd = batch_of(deg)
    for flag in FLAGS:
        got = {form: _with_form(form, lambda: run(rd, INFIX | flag, None)) for form in FORMS}
        assert got["0"] == got["1"]
        assert [got["0"][i] for i in sample] == [tuple(I.locate(*deg[i], INFIX, flag)) for i in sample]
        worse = [i for i in range(len(pairs)) if got["0"][i][0] > unbounded[i][0]]
        assert not worse, (len(worse), worse[:8])
    rd.close()


@pytest.mark.parametrize("form", FORMS)
def test_n_on_either_side(form, monkeypatch):
    rng = np.random.default_rng(G.SEED + 9)
    p = bytes(M._rand(rng, 40))
    pairs = [(p, b"N" * 300), (b"N" * 40, bytes(M._rand(rng, 300))), (b"n" * 70, b"N" * 300)]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        a = run_and_compare(rb, pairs, mode, IUPAC, None)
        assert a[0] == (0, 0, 40) and a[1] == (0, 0, 40) and a[2] == (0, 0, 70)           # a text N matches every pattern symbol
        b = run_and_compare(rb, pairs, mode, IUPAC_PATTERN, None)
        assert b[0][0] == 40 and b[1] == (0, 0, 40) and b[2][0] == 70                     # ... unless the text is read as ACGT only
        assert rb.run_search(mode, None) == capi.QUICKED_OK                               # unflagged: N is one symbol, equal to itself only
        assert results(rb)[0] == [S.locate(x, t, mode) for x, t in pairs]
    rb.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches_equal_the_ascii_batch(wire, form, monkeypatch):
    if wire == capi.WIRE_2BIT:
        pairs = M.grid_cases()[::3] + M.tie_cases()
    else:
        pairs = [c for c in G.grid_cases() + G.random_cases()[:120] if set(c[0]) | set(c[1]) <= set(b"ACGTN")]
        assert len(pairs) > 60 and any(b"N" in p for p, _ in pairs) and any(b"N" in t for _, t in pairs)
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb, ra = batch_of(pairs, wire=wire), batch_of(pairs)
    for flag in FLAGS:
        for mode in MODES:
            bounds = cycle_bounds(pairs, mode, flag)
            run_and_compare(rb, pairs, mode, flag, bounds)
            assert ra.run_search(mode | flag, np.array(bounds, dtype=np.int32)) == capi.QUICKED_OK
            assert results(ra)[0] == results(rb)[0]
        assert rb.run_search_all(INFIX | flag, 12, max_hits=4) == capi.QUICKED_OK and ra.run_search_all(INFIX | flag, 12, max_hits=4) == capi.QUICKED_OK
        assert hits_of(rb) == hits_of(ra)
    if wire == capi.WIRE_2BIT:                       # ACGT only: the flagged run is the unflagged one
        assert rb.run_search(INFIX | IUPAC, None) == capi.QUICKED_OK
        flagged = results(rb)[0]
        assert rb.run_search(INFIX, None) == capi.QUICKED_OK
        assert results(rb)[0] == flagged
    rb.close()
    ra.close()


@pytest.mark.parametrize("form", FORMS)
def test_queued_run_and_fetch_equal_the_sync_run(form, monkeypatch):
    pairs = G.grid_cases()[1::3] + G.named_cases()
    half = pairs[::2]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    a, b = batch_of(pairs), batch_of(half)
    for flag in FLAGS:
        for mode in MODES:
            bounds = cycle_bounds(pairs, mode, flag)
            run_and_compare(a, pairs, mode, flag, bounds, sync=True)
            run_and_compare(a, pairs, mode, flag, bounds, sync=False)
            # two queued runs of different batches, one flagged and one not, fetched in the other order
            assert a.run_search(mode | flag, 5, sync=False) == capi.QUICKED_OK
            assert b.run_search(mode, None, sync=False) == capi.QUICKED_OK
            assert b.fetch() == capi.QUICKED_OK and a.fetch() == capi.QUICKED_OK
            assert results(a)[0] == expect(pairs, mode, flag, [5] * len(pairs))
            assert results(b)[0] == [S.locate(p, t, mode) for p, t in half]
    a.close()
    b.close()


@pytest.mark.parametrize("form", FORMS)
def test_argument_rules_unimplemented_and_unflagged_runs_around_a_flagged_one(form, monkeypatch):
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    pairs = [(b"ACGYN", b"TTACGCGTT"), (b"", b"ACGT"), (b"ACGT", b""), (b"RRRR", b"YYYY")] + G.grid_cases()[40:80]
    rb = batch_of(pairs)
    for mode in (0, 3, 16, 16 | 3, 16 | 32 | 2, 64 | 2):
        assert rb.run_search(mode, 3) == capi.QUICKED_ERROR
        assert rb.run_search_all(mode, 3, max_hits=4) == capi.QUICKED_ERROR
    with pytest.raises(capi.QuickedException):
        rb.locations()                                              # nothing ran
    for flag in FLAGS:
        assert rb.run_search(INFIX | flag, 2, only_score=False) == capi.QUICKED_UNIMPLEMENTED
        assert rb.run_search(INFIX | flag, 2, only_score=False, sync=False) == capi.QUICKED_UNIMPLEMENTED
        assert rb.configure(cigar_style=0, check=True) == capi.QUICKED_OK
        assert rb.run_search(INFIX | flag, 2) == capi.QUICKED_UNIMPLEMENTED
        assert rb.run_search_all(INFIX | flag, 2, max_hits=4) == capi.QUICKED_UNIMPLEMENTED
        assert rb.configure(cigar_style=0, check=False) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.locations()                                              # nothing was queued
    # an unflagged run before and after a flagged one: its old results, the same work
    for mode in MODES:
        assert rb.run_search(mode, None) == capi.QUICKED_OK
        before, steps = results(rb)[0], int(rb.counters()[0])
        assert before == [(-1, -1, -1) if not p or not t else S.locate(p, t, mode) for p, t in pairs]
        for flag in FLAGS:
            exp = run_and_compare(rb, pairs, mode, flag, None)
            assert exp[0] == ((0, 2, 7) if mode == INFIX else (2, 0, 7)) and exp[3][0] == 4      # Y = C, N = G (PREFIX pays for the TT in front); R and Y share no base
        assert rb.run_search(mode, None) == capi.QUICKED_OK
        assert results(rb)[0] == before and int(rb.counters()[0]) == steps
    rb.close()
