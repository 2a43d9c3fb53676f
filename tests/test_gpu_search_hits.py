"""Every occurrence within the bound on the GPU (quicked_batch_run_search_all through capi.ResidentBatch).  Expected values
never come from the library: the brute force of tests/search_hits_lib.py -- the definition, computed live, once per (pair,
mode) and shared -- and the best search's own brute force (search_lib.locate).  Every test runs in both kernel forms through
QE_SEARCH_FORM where both apply."""
import importlib.util
import os

import numpy as np
import pytest

import search_hits_lib as H
import search_lib as S
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = capi.SEARCH_PREFIX, capi.SEARCH_INFIX
MODES = [PREFIX, INFIX]
FORMS = ["0", "1"]                               # QE_SEARCH_FORM: the workspace form always / the register form where it applies
INT_MAX = 2**31 - 1


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_hits_cases", os.path.join(ROOT, "tests", "golden", "make_search_hits_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _cases()
M = G.M
_BEST = {}


def best_search(p, t, mode):
    key = (p, t, mode)
    if key not in _BEST:
        _BEST[key] = S.locate(p, t, mode)
    return _BEST[key]


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
    """-> (found, [[(start, end, score)] per pair], scores, statuses)"""
    found, off, hits = rb.hits()
    sc, st = rb.scores()
    assert off[0] == 0 and off[-1] == len(hits) and (np.diff(off) >= 0).all()
    rows = list(zip(hits["text_start"].tolist(), hits["text_end"].tolist(), hits["score"].tolist()))
    return found.tolist(), [rows[off[i]:off[i + 1]] for i in range(len(found))], sc.tolist(), st.tolist()


def per_pair(bounds, n):
    if bounds is None:
        return [INT_MAX] * n
    return [int(bounds)] * n if np.ndim(bounds) == 0 else [int(b) for b in bounds]


def run_and_compare(rb, pairs, mode, bounds, cap):
    """bounds: None, one int, or one per pair; -> the brute force's lists"""
    bd = per_pair(bounds, len(pairs))
    exp = [H.occurrences(p, t, mode, b) if p and t else [] for (p, t), b in zip(pairs, bd)]
    arg = bounds if (bounds is None or np.ndim(bounds) == 0) else np.asarray(bounds, dtype=np.int32)
    assert rb.run_search_all(mode, arg, max_hits=cap) == capi.QUICKED_OK
    found, lists, sc, st = results(rb)
    bad = [(i, len(pairs[i][0]), len(pairs[i][1]), bd[i], found[i], lists[i][:3], exp[i][:3]) for i in range(len(pairs))
           if found[i] != len(exp[i]) or lists[i] != exp[i][:cap]]
    assert not bad, (len(bad), bad[:6])
    # the scores: the smallest among ALL found occurrences, -1 without one; the statuses
    assert sc == [min(o[2] for o in e) if e else -1 for e in exp]
    assert st == [capi.QUICKED_OK if p and t else capi.QUICKED_EMPTY_SEQUENCE for p, t in pairs]
    return exp


def cycle_bounds(pairs, mode):
    """0, 1, d - 1, d, d + 1, 63, 64 and m in turn"""
    out = []
    for i, (p, t) in enumerate(pairs):
        d = best_search(p, t, mode)[0]
        out.append((0, 1, max(0, d - 1), d, d + 1, 63, 64, len(p))[i % 8])
    return out


def shape_pairs():
    return [q for name in ("grid", "ties", "borders", "edges", "short", "adjacent", "lengths", "symbols") for q in G.SETS[name]()]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_grid_ties_and_border_sets(mode, form, monkeypatch):
    pairs = shape_pairs()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    rb.kernel_times()
    exp = run_and_compare(rb, pairs, mode, cycle_bounds(pairs, mode), 16)
    _, launches = rb.kernel_times()
    assert launches[0] >= (2 if mode == INFIX else 1) and rb.counters()[0] > 0      # the passes: slot [0] of both
    assert sum(1 for e in exp if len(e) > 1) * 8 >= len(exp) and any(not e for e in exp)
    for k in (3, 64):
        run_and_compare(rb, pairs, mode, k, 16)
    with pytest.raises(capi.QuickedException):
        rb.locations()                                              # no locations, no strings
    assert all(c is None for c in rb.cigars())
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_tandem_repeats_under_caps(form, monkeypatch):
    """dozens of occurrences per pair: found is the same under every cap, the stored lists are prefixes of each other; and the
    start pass in slices of one group (QE_SEARCH_HITS_WS_KB) gives what one launch gives"""
    pairs = G.SETS["tandem"]()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        got = {}
        for cap in (1, 2, 64):
            exp = run_and_compare(rb, pairs, mode, 3, cap)
            got[cap] = results(rb)
        if mode == INFIX:
            assert all(24 <= len(e) for e in exp) and any(len(e) > 2 for e in exp)
        assert got[1][0] == got[2][0] == got[64][0]
        assert all(a == c[:1] and b == c[:2] for a, b, c in zip(got[1][1], got[2][1], got[64][1]))
        assert got[1][2] == got[64][2]                              # the scores do not know the cap
    monkeypatch.setenv("QE_SEARCH_HITS_WS_KB", "1")
    exp = run_and_compare(rb, pairs, INFIX, 3, 64)
    assert sum(min(64, len(e)) for e in exp) > 128                  # more than two groups of occurrences: more than two slices
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_dead_blocks_between_occurrences(form, monkeypatch):
    """1 000-base patterns (the workspace form under either switch): two occurrences 1 600 columns apart and a decoy just
    beyond the bound; at the set's own bound the lower blocks die in between and enter again"""
    pairs = G.SETS["dead"]()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    exp = run_and_compare(rb, pairs, INFIX, G.DEAD_BOUND, 8)
    assert all(len(e) == 2 for e in exp)
    steps_bound = rb.counters()[0]
    exp = run_and_compare(rb, pairs, INFIX, None, 64)
    assert all(len(e) > 2 for e in exp) and 2 * steps_bound < rb.counters()[0]
    run_and_compare(rb, pairs, PREFIX, G.DEAD_BOUND, 8)
    rb.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_wave_shapes(count, form, monkeypatch):
    """mixed lengths in one wave, pairs without an occurrence, empty sequences in the middle of a wave"""
    src = M.random_cases(G.RANDOM_COUNT)
    pairs = [(p, t) for p, t, _, _ in src[:count]]
    bounds = [bd for _, _, _, bd in src[:count]]
    if count > 2:
        pairs[count // 2] = (b"", pairs[count // 2][1])
        pairs[count // 3] = (pairs[count // 3][0], b"")
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        exp = run_and_compare(rb, pairs, mode, bounds, 4)
        if count >= 63:
            assert any(not e for e, (p, t) in zip(exp, pairs) if p and t) and any(len(e) > 4 for e in exp)
        run_and_compare(rb, pairs, mode, 7, 4)                      # max_dist_all against the per-pair bounds above
    rb.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches_equal_the_ascii_batch(wire, form, monkeypatch):
    pairs = G.SETS["grid"]()[::2] + G.SETS["ties"]() + G.SETS["adjacent"]()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb, ra = batch_of(pairs, wire=wire), batch_of(pairs)
    for mode in MODES:
        bounds = cycle_bounds(pairs, mode)
        run_and_compare(rb, pairs, mode, bounds, 8)
        assert ra.run_search_all(mode, np.array(bounds, dtype=np.int32), max_hits=8) == capi.QUICKED_OK
        assert results(ra) == results(rb)
    rb.close()
    ra.close()


@pytest.mark.parametrize("form", FORMS)
def test_the_smallest_occurrence_is_the_best_search_answer(form, monkeypatch):
    """on the same batch object with the same bounds: the smallest score among a pair's occurrences and the first occurrence
    that has it are quicked_batch_run_search's {score, text_start, text_end}, d == m included; and the scores of a capped
    run are those of the uncapped one"""
    pairs = shape_pairs() + M.no_similarity_cases() + G.SETS["tandem"]()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        for bounds in (np.array(cycle_bounds(pairs, mode), dtype=np.int32), None):
            assert rb.run_search(mode, bounds) == capi.QUICKED_OK
            sc, _ = rb.scores()
            ts, te = rb.locations()
            best = list(zip(sc.tolist(), ts.tolist(), te.tolist()))
            assert rb.run_search_all(mode, bounds, max_hits=4096) == capi.QUICKED_OK
            found, lists, sc_all, _ = results(rb)
            assert found == [len(x) for x in lists]                 # nothing capped
            assert [H.best_of([(s, e, v) for s, e, v in x]) for x in lists] == best
            assert sc_all == [b[0] for b in best]
            assert rb.run_search_all(mode, bounds, max_hits=1) == capi.QUICKED_OK
            found1, lists1, sc1, _ = results(rb)
            assert sc1 == sc_all and found1 == found and lists1 == [x[:1] for x in lists]
            assert any(x and x[0][2] > s for x, s in zip(lists1, sc1))      # a stored occurrence that is not the best one
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_every_stored_stretch_is_the_longest_of_its_score(form, monkeypatch):
    """INFIX: the stretch text[start:end] of every stored occurrence has global distance `score` to the pattern, and the
    stretch one base longer to the left does not"""
    pairs = G.SETS["ties"]() + G.SETS["adjacent"]() + G.SETS["borders"]() + G.SETS["symbols"]() + G.SETS["tandem"]()[:1]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    assert rb.run_search_all(INFIX, None, max_hits=32) == capi.QUICKED_OK
    _, lists, _, _ = results(rb)
    checked = 0
    for (p, t), occ in zip(pairs, lists):
        for s, e, v in occ:
            assert 0 <= s < e <= len(t)
            assert int(S.last_row(p, t[s:e], True)[-1]) == v, (len(p), s, e, v)
            if s > 0:
                assert int(S.last_row(p, t[s - 1:e], True)[-1]) != v, (len(p), s, e, v)
            checked += 1
    assert checked > 200
    rb.close()


def test_batch_at_size():
    """20 000 pairs of a 150-base pattern in a 400-base text at 4 %, bound 12, cap 4: the two forms give identical results on
    all pairs, and the brute force's on the seeded sample of 200"""
    pairs = M.big_batch()
    assert len(pairs) == M.BIG["count"]
    sample = M.big_sample_indices()
    bound = M.BIG["bound"]
    rb = batch_of(pairs)
    for mode in (INFIX, PREFIX):
        got = {}
        for form in FORMS:
            os.environ["QE_SEARCH_FORM"] = form
            capi.reload_env()
            try:
                assert rb.run_search_all(mode, bound, max_hits=4) == capi.QUICKED_OK
                got[form] = results(rb)
            finally:
                del os.environ["QE_SEARCH_FORM"]
                capi.reload_env()
        assert got["0"] == got["1"]
        found, lists, sc, _ = got["0"]
        exp = [H.occurrences(*pairs[i], mode, bound) for i in sample]
        assert [found[i] for i in sample] == [len(e) for e in exp]
        assert [lists[i] for i in sample] == [e[:4] for e in exp]
        if mode == INFIX:
            assert sum(1 for e in exp if e) * 2 >= len(exp)
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_unimplemented_and_error_cases(form, monkeypatch):
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    pairs = [(b"ACGT", b"TTACGATTACGTT"), (b"", b"ACGT"), (b"ACGT", b""), (b"AAAA", b"TTTT")]
    rb = batch_of(pairs)
    with pytest.raises(capi.QuickedException):
        rb.hits()                                                   # no run yet
    assert rb.run_search_all(INFIX, np.array([1, 1, -1, 1], dtype=np.int32)) == capi.QUICKED_ERROR
    assert rb.run_search_all(INFIX, -3) == capi.QUICKED_ERROR
    assert rb.run_search_all(0, 3) == capi.QUICKED_ERROR and rb.run_search_all(3, 3) == capi.QUICKED_ERROR
    assert rb.run_search_all(INFIX, 3, max_hits=0) == capi.QUICKED_ERROR
    assert rb.run_search_all(INFIX, 3, max_hits=4097) == capi.QUICKED_ERROR
    assert rb.run_search_all(INFIX, 2, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(cigar_style=0, check=True) == capi.QUICKED_OK
    assert rb.run_search_all(INFIX, 2) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(cigar_style=0, check=False) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.hits()
    assert rb.configure_tags(stats=True) == capi.QUICKED_OK         # ignored: these runs produce no alignments
    assert rb.run_search_all(INFIX, 1, max_hits=4) == capi.QUICKED_OK
    found, lists, sc, st = results(rb)
    assert lists[0] == H.occurrences(*pairs[0], INFIX, 1) and lists[1:] == [[], [], []]
    assert [o[2] for o in lists[0]] == [1, 0] and lists[0][1] == (8, 12, 0)      # ACGA with one edit, then ACGT itself
    assert found == [2, 0, 0, 0] and sc == [0, -1, -1, -1]
    assert st == [capi.QUICKED_OK, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_OK]
    with pytest.raises(capi.QuickedException):
        rb.pair_stats()
    assert rb.configure_tags() == capi.QUICKED_OK
    # a best-search run and a bounded run afterwards make the new getters refuse
    assert rb.run_search(INFIX, None) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.hits()
    assert rb.run_search_all(PREFIX, None, max_hits=4) == capi.QUICKED_OK
    assert results(rb)[1][0] == H.occurrences(*pairs[0], PREFIX, 4)
    assert rb.run_bounded(3) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.hits()
    rb.close()
