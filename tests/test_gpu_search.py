"""Approximate pattern search on the GPU (quicked_batch_run_search through capi.ResidentBatch).  Expected values never come
from the library: the brute-force DP of tests/search_lib.py (the definition, computed live) and, for the batch at size,
edlib's recorded answers (tests/golden/search_cases.json).  Every test runs in both kernel forms through QE_SEARCH_FORM
where both apply."""
import importlib.util
import os

import numpy as np
import pytest

import check_lib as K
import oracle_lib as O
import search_lib as S
import tags_lib as T
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = capi.SEARCH_PREFIX, capi.SEARCH_INFIX
MODES = [PREFIX, INFIX]
FORMS = ["0", "1"]                               # QE_SEARCH_FORM: the workspace form always / the register form where it applies
INT_MAX = 2**31 - 1


def _cases():
    spec = importlib.util.spec_from_file_location("make_search_cases", os.path.join(ROOT, "tests", "golden", "make_search_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _cases()
_BF = {}


def brute(p, t, mode):
    """(d, start, end) without a bound; computed once per (pair, mode) and shared"""
    key = (p, t, mode)
    if key not in _BF:
        _BF[key] = S.locate(p, t, mode)
    return _BF[key]


def expect(pairs, mode, bounds):
    out = []
    for (p, t), bd in zip(pairs, bounds):
        out.append((-1, -1, -1) if not p or not t else S.bounded(brute(p, t, mode), len(p), bd))
    return out


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


def run_and_compare(rb, pairs, mode, bounds, sync=True):
    """bounds: None, one int, or one per pair"""
    if bounds is None:
        per_pair = [INT_MAX] * len(pairs)
    elif np.ndim(bounds) == 0:
        per_pair = [int(bounds)] * len(pairs)
    else:
        per_pair = [int(b) for b in bounds]
    exp = expect(pairs, mode, per_pair)
    arg = bounds if (bounds is None or np.ndim(bounds) == 0) else np.asarray(bounds, dtype=np.int32)
    assert rb.run_search(mode, arg, only_score=True, sync=sync) == capi.QUICKED_OK
    if not sync:
        assert rb.fetch() == capi.QUICKED_OK
    got, status = results(rb)
    bad = [(i, len(pairs[i][0]), len(pairs[i][1]), per_pair[i], got[i], exp[i]) for i in range(len(pairs)) if got[i] != tuple(exp[i])]
    assert not bad, (len(bad), bad[:8])
    want_status = [capi.QUICKED_OK if p and t else capi.QUICKED_EMPTY_SEQUENCE for p, t in pairs]
    assert status.tolist() == want_status
    assert all(c is None for c in rb.cigars())
    return exp


def cycle_bounds(pairs, mode):
    """0, 1, d - 1, d, d + 1, 63, 64 and m in turn"""
    out = []
    for i, (p, t) in enumerate(pairs):
        d = brute(p, t, mode)[0]
        out.append((0, 1, max(0, d - 1), d, d + 1, 63, 64, len(p))[i % 8])
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_grid_and_ties(mode, form, monkeypatch):
    pairs = M.grid_cases() + M.tie_cases() + M.no_similarity_cases()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    rb.kernel_times()
    run_and_compare(rb, pairs, mode, None)
    _, launches = rb.kernel_times()
    assert launches[0] >= (2 if mode == INFIX else 1) and rb.counters()[0] > 0      # the search passes: slot [0] of both
    exp = run_and_compare(rb, pairs, mode, cycle_bounds(pairs, mode))
    within = sum(1 for e in exp if e[0] >= 0)
    assert within * 4 >= len(exp) and (len(exp) - within) * 4 >= len(exp)
    for k in (3, 64):
        run_and_compare(rb, pairs, mode, k)
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_live_block_cases(form, monkeypatch):
    """patterns of 1 000 and 3 000 bases behind a decoy just beyond the bound, with and without two indels: every real
    occurrence is found at its case's bound (per-pair bounds), and the runs at 20, 100 and without a bound equal the brute force"""
    cases = M.live_cases()
    pairs = [(c[0], c[1]) for c in cases]
    own = [c[2] for c in cases]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    exp = run_and_compare(rb, pairs, INFIX, own)
    assert all(e[0] > 0 and e[2] > c[3] for e, c in zip(exp, cases))          # within the bound, and not the decoy
    for bd in M.LIVE_BOUNDS + (INT_MAX,):
        run_and_compare(rb, pairs, INFIX, bd)
    rb.close()
    short = [q for q in pairs if len(q[0]) == 1000]          # PREFIX: the 1 000-base cases (the reference DP of the others is the slow part)
    rb = batch_of(short)
    for bd in M.LIVE_BOUNDS + (INT_MAX,):
        run_and_compare(rb, short, PREFIX, bd)
    rb.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_wave_shapes(count, form, monkeypatch):
    """mixed lengths in one wave, pairs that are beyond, empty sequences in the middle of a wave"""
    src = M.random_cases()
    pairs = [(p, t) for p, t, _, _ in src[:count]]
    bounds = [bd for _, _, _, bd in src[:count]]
    if count > 2:
        pairs[count // 2] = (b"", pairs[count // 2][1])
        pairs[count // 3] = (pairs[count // 3][0], b"")
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    for mode in MODES:
        exp = run_and_compare(rb, pairs, mode, bounds)
        if count >= 63:
            assert any(e[0] < 0 for e, (p, t) in zip(exp, pairs) if p and t) and any(e[0] >= 0 for e in exp)
        run_and_compare(rb, pairs, mode, 7)                       # max_dist_all against the per-pair bounds above
    rb.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wire", [capi.WIRE_2BIT, capi.WIRE_PLANES3])
def test_packed_batches_equal_the_ascii_batch(wire, form, monkeypatch):
    pairs = M.grid_cases()[::2] + M.tie_cases()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb, ra = batch_of(pairs, wire=wire), batch_of(pairs)
    for mode in MODES:
        bounds = cycle_bounds(pairs, mode)
        run_and_compare(rb, pairs, mode, bounds)
        assert ra.run_search(mode, np.array(bounds, dtype=np.int32)) == capi.QUICKED_OK
        assert results(ra)[0] == results(rb)[0]
    rb.close()
    ra.close()


@pytest.mark.parametrize("form", FORMS)
def test_queued_run_and_fetch_equal_the_sync_run(form, monkeypatch):
    pairs = M.grid_cases()[1::3] + M.tie_cases()
    half = pairs[::2]
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    a, b = batch_of(pairs), batch_of(half)
    for mode in MODES:
        bounds = cycle_bounds(pairs, mode)
        run_and_compare(a, pairs, mode, bounds, sync=True)
        run_and_compare(a, pairs, mode, bounds, sync=False)
        # two queued runs of different batches, fetched in the other order
        assert a.run_search(mode, 5, sync=False) == capi.QUICKED_OK
        assert b.run_search(mode, None, sync=False) == capi.QUICKED_OK
        assert b.fetch() == capi.QUICKED_OK and a.fetch() == capi.QUICKED_OK
        assert results(a)[0] == [tuple(e) for e in expect(pairs, mode, [5] * len(pairs))]
        assert results(b)[0] == [tuple(e) for e in expect(half, mode, [INT_MAX] * len(half))]
    a.close()
    b.close()


def _edits(cigar):
    return sum(n for o, n in T.parse_cigar(cigar) if o != 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_cigars_statistics_and_md(mode, form, monkeypatch):
    pairs = M.grid_cases()[::2] + M.tie_cases()
    bounds = cycle_bounds(pairs, mode)
    exp = expect(pairs, mode, bounds)
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    rb = batch_of(pairs)
    assert rb.configure_tags(stats=True, md=True) == capi.QUICKED_OK
    assert rb.run_search(mode, np.array(bounds, dtype=np.int32), only_score=False, sync=True) == capi.QUICKED_OK
    got, status = results(rb)
    assert got == [tuple(e) for e in exp] and (status == capi.QUICKED_OK).all()
    cig, stats, md = rb.cigars(), rb.pair_stats(), rb.md()
    for i, (p, t) in enumerate(pairs):
        d, s, e = exp[i]
        if d < 0:
            assert cig[i] is None and md[i] is None and (stats[i] == -1).all(), i
            continue
        assert cig[i] is not None, i
        assert K.verdict(p, t[s:e], cig[i]) == 1, (i, cig[i], s, e)          # the Python walk, against the located stretch
        assert _edits(cig[i]) == d, (i, cig[i], d)
        ops = T.parse_cigar(cig[i])
        st = T.stats(ops)
        assert tuple(stats[i].tolist()) == tuple(st), (i, stats[i].tolist(), st)
        assert T.identities_hold(st, len(p), e - s, d), (i, st)              # ins_bases + matches + mismatches = the stretch
        assert md[i].encode("latin-1") == T.md(ops, p), (i, md[i])
    # the SAM styles, and a run without strings
    ref = cig
    assert rb.configure_tags() == capi.QUICKED_OK
    assert rb.configure(cigar_style=1) == capi.QUICKED_OK
    assert rb.run_search(mode, np.array(bounds, dtype=np.int32), only_score=False) == capi.QUICKED_OK
    for i, c in enumerate(rb.cigars()):
        assert (c is None) == (ref[i] is None)
        if c is not None:
            assert c == O.sam_cigar(ref[i], True), (i, c, ref[i])
    assert rb.configure(cigar_style=0) == capi.QUICKED_OK
    assert rb.configure_tags(stats=True, cigar=False) == capi.QUICKED_OK
    assert rb.run_search(mode, np.array(bounds, dtype=np.int32), only_score=False) == capi.QUICKED_OK
    assert all(c is None for c in rb.cigars()) and (rb.pair_stats() == stats).all()
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_non_canonical_pairs_are_located_but_carry_no_cigar(form, monkeypatch):
    pairs = M.symbol_cases()
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    noncanon = [any(c not in b"ACGTN" for c in p + t) for p, t in pairs]
    assert any(noncanon) and not all(noncanon)
    rb = batch_of(pairs)
    assert rb.configure_tags(stats=True, md=True) == capi.QUICKED_OK
    for mode in MODES:
        exp = expect(pairs, mode, [INT_MAX] * len(pairs))
        assert rb.run_search(mode, None, only_score=False) == capi.QUICKED_OK
        got, status = results(rb)
        assert got == [tuple(e) for e in exp] and (status == capi.QUICKED_OK).all()
        cig, stats, md = rb.cigars(), rb.pair_stats(), rb.md()
        for i, (p, t) in enumerate(pairs):
            if noncanon[i]:
                assert cig[i] is None and md[i] is None and (stats[i] == -1).all(), i
            else:
                d, s, e = exp[i]
                assert K.verdict(p, t[s:e], cig[i]) == 1 and _edits(cig[i]) == d, (i, cig[i])
    rb.close()


@pytest.mark.parametrize("form", FORMS)
def test_unimplemented_and_error_cases(form, monkeypatch):
    monkeypatch.setenv("QE_SEARCH_FORM", form)
    pairs = [(b"ACGT", b"TTACGATT"), (b"", b"ACGT"), (b"ACGT", b""), (b"AAAA", b"TTTT")]
    rb = batch_of(pairs)
    with pytest.raises(capi.QuickedException):
        rb.locations()                                              # no run yet
    assert rb.run_search(INFIX, np.array([1, 1, -1, 1], dtype=np.int32)) == capi.QUICKED_ERROR
    assert rb.run_search(INFIX, -3) == capi.QUICKED_ERROR
    assert rb.run_search(0, 3) == capi.QUICKED_ERROR and rb.run_search(3, 3) == capi.QUICKED_ERROR
    assert rb.run_search(INFIX, 2, only_score=False, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(cigar_style=0, check=True) == capi.QUICKED_OK
    assert rb.run_search(INFIX, 2) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_search(INFIX, 2, only_score=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.configure(cigar_style=0, check=False) == capi.QUICKED_OK
    assert rb.run_search(INFIX, 2) == capi.QUICKED_OK
    got, status = results(rb)
    assert got == [S.bounded(S.locate(*pairs[0], INFIX), 4, 2), (-1, -1, -1), (-1, -1, -1), (-1, -1, -1)] and got[0][0] == 1
    assert status.tolist() == [capi.QUICKED_OK, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_OK]
    # the getter refuses after a run that was not a search run, and after a bounded one
    assert rb.run(capi.make_params(algo=capi.BANDED, only_score=True), sync=True) >= 0
    with pytest.raises(capi.QuickedException):
        rb.locations()
    assert rb.run_search(PREFIX, None) == capi.QUICKED_OK
    assert results(rb)[0][0] == S.locate(b"ACGT", b"TTACGATT", PREFIX)
    assert rb.run_bounded(3) == capi.QUICKED_OK
    with pytest.raises(capi.QuickedException):
        rb.locations()
    rb.close()


def test_batch_at_size():
    """20 000 pairs of a 150-base pattern in a 400-base text at 4 %, bound 12: the two forms give identical answers on all
    pairs, and edlib's recorded answers on a seeded sample of 200"""
    pairs = M.big_batch()
    assert len(pairs) == M.BIG["count"]
    sample, rec = M.big_sample_indices(), M.expected("big_sample")
    bound = M.BIG["bound"]
    rb = batch_of(pairs)
    for mode, col in ((INFIX, 1), (PREFIX, 0)):
        exp = [tuple(r[col]) if r[col][0] <= bound else (-1, -1, -1) for r in rec]
        if mode == INFIX:
            assert sum(1 for e in exp if e[0] >= 0) * 2 >= len(exp)
        got = {}
        for form in FORMS:
            os.environ["QE_SEARCH_FORM"] = form
            capi.reload_env()
            try:
                assert rb.run_search(mode, bound) == capi.QUICKED_OK
                got[form] = results(rb)[0]
            finally:
                del os.environ["QE_SEARCH_FORM"]
                capi.reload_env()
        assert got["0"] == got["1"]
        assert [got["0"][i] for i in sample] == exp
    rb.close()
