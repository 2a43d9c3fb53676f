"""Bounded edit distance on the GPU (quicked_batch_run_bounded through capi.ResidentBatch).  Expected values never come
from the library: edlib's distances (tests/golden/bounded_cases.json, live where oracle/_ref is built) thresholded here;
for pairs with lower-case / IUPAC bytes the compiled reference's QUICKED score.  Every batch must have at least a quarter
of its live pairs within their bound and a quarter beyond -- asserted on the expected values before the library's are
looked at."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    spec = importlib.util.spec_from_file_location("make_bounded_cases", os.path.join(ROOT, "tests", "golden", "make_bounded_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _cases()
WIRES = [None, capi.WIRE_2BIT, capi.WIRE_PLANES3]
SWITCHES = [None, "0", "1"]


def _pools(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs) or b"\0", dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1])]).astype(np.int64)
    return pp, po, pl, tp, to, tl


def _balanced(exp):
    exp = np.asarray(exp)
    n, within = len(exp), int((exp >= 0).sum())
    assert within * 4 >= n and (n - within) * 4 >= n, f"one-sided batch: {within} of {n} within"


def _set_switch(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("QE_BOUNDED_DIAG", raising=False)
    else:
        monkeypatch.setenv("QE_BOUNDED_DIAG", value)


def _check_form(rb, switch, any_diag_eligible):
    """slot [3] of kernel_times: the diagonal-word launches since the last call"""
    _, launches = rb.kernel_times()
    if switch == "1" and any_diag_eligible:
        assert launches[3] > 0, launches
    if switch == "0":
        assert launches[3] == 0, launches
    return launches


def _for_wire(pairs, wire):
    """indices of the pairs the wire format can hold (2BIT: no N)"""
    if wire == capi.WIRE_2BIT:
        return [i for i, (p, t) in enumerate(pairs) if b"N" not in p and b"N" not in t]
    return list(range(len(pairs)))


_grid = {}


def grid():
    if not _grid:
        pairs = M.grid_pairs()
        _grid["pairs"], _grid["dist"] = pairs, M.expected("grid", pairs)
    return _grid["pairs"], _grid["dist"]


def _run_and_compare(rb, bounds, exp, sync=True):
    st = rb.run_bounded(bounds, only_score=True, sync=sync)
    assert st == capi.QUICKED_OK, st
    if not sync:
        assert rb.fetch() == capi.QUICKED_OK
    scores, status = rb.scores()
    bad = np.nonzero(scores != np.asarray(exp, dtype=np.int32))[0]
    assert len(bad) == 0, [(int(i), int(scores[i]), int(exp[i]), int(np.asarray(bounds).reshape(-1)[i % np.size(bounds)])) for i in bad[:10]]
    assert (status == capi.QUICKED_OK).all()
    assert all(c is None for c in rb.cigars())


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("wire", WIRES)
def test_grid_and_bound_sweep_as_one_ragged_batch(wire, switch, monkeypatch):
    """every grid pair at every bound 0 .. 63: one batch entry per (pair, bound), a per-pair bound array"""
    pairs, dist = grid()
    keep = _for_wire(pairs, wire)
    ent = [(i, k) for i in keep for k in range(M.MAX_DIAG + 1)]
    exp = [M.threshold(dist[i], k) for i, k in ent]
    _balanced(exp)
    _set_switch(monkeypatch, switch)
    rb = capi.ResidentBatch(datagen.PairBatch(*_pools([pairs[i] for i, _ in ent])), wire=wire)
    rb.kernel_times()
    _run_and_compare(rb, np.array([k for _, k in ent], dtype=np.int32), exp)
    _check_form(rb, switch, True)
    rb.close()


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("wire", WIRES)
def test_mixed_per_pair_bounds(wire, switch, monkeypatch):
    """0, small, 63, 64, 65, 100, 1000 and bounds above max(m, n) in one batch"""
    pairs, dist = grid()
    bounds = M.mixed_bounds(pairs)
    keep = _for_wire(pairs, wire)
    exp = [M.threshold(dist[i], bounds[i]) for i in keep]
    _balanced(exp)
    assert {0, 63, 64, 65, 100, 1000} <= {bounds[i] for i in keep}
    assert any(bounds[i] > max(len(pairs[i][0]), len(pairs[i][1])) for i in keep)
    _set_switch(monkeypatch, switch)
    rb = capi.ResidentBatch(datagen.PairBatch(*_pools([pairs[i] for i in keep])), wire=wire)
    rb.kernel_times()
    _run_and_compare(rb, np.array([bounds[i] for i in keep], dtype=np.int32), exp)
    _check_form(rb, switch, True)
    # one bound for the whole batch
    for k in (45, 63, 64, 90):
        e = [M.threshold(dist[i], k) for i in keep]
        _balanced(e)
        _run_and_compare(rb, k, e)
    rb.close()


def test_argument_checks_and_empty_sequences():
    pairs = [(b"ACGT", b"ACGA"), (b"", b"ACGT"), (b"ACGT", b""), (b"AAAA", b"TTTT")]
    rb = capi.ResidentBatch(datagen.PairBatch(*_pools(pairs)))
    assert rb.run_bounded(np.array([1, 1, -1, 1], dtype=np.int32)) == capi.QUICKED_ERROR
    assert rb.run_bounded(-3) == capi.QUICKED_ERROR
    assert rb.run_bounded(2, only_score=False, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_bounded(2) == capi.QUICKED_OK
    scores, status = rb.scores()
    assert scores.tolist() == [1, -1, -1, -1]
    assert status.tolist() == [capi.QUICKED_OK, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_EMPTY_SEQUENCE, capi.QUICKED_OK]
    rb.close()


@pytest.mark.parametrize("switch", SWITCHES)
def test_queued_runs_and_fetch(switch, monkeypatch):
    """sync == 0 + quicked_batch_fetch gives what sync != 0 gives; two queued runs of different batches, fetched in the
    other order"""
    pairs, dist = grid()
    bounds = np.array(M.mixed_bounds(pairs), dtype=np.int32)
    exp_a = [M.threshold(d, k) for d, k in zip(dist, bounds)]
    half = [i for i in range(len(pairs)) if i % 2]
    exp_b = [M.threshold(dist[i], 63) for i in half]
    _balanced(exp_a)
    _balanced(exp_b)
    _set_switch(monkeypatch, switch)
    a = capi.ResidentBatch(datagen.PairBatch(*_pools(pairs)))
    b = capi.ResidentBatch(datagen.PairBatch(*_pools([pairs[i] for i in half])))
    _run_and_compare(a, bounds, exp_a, sync=True)
    _run_and_compare(a, bounds, exp_a, sync=False)
    a.kernel_times()
    assert a.run_bounded(bounds, sync=False) == capi.QUICKED_OK
    assert b.run_bounded(63, sync=False) == capi.QUICKED_OK
    assert b.fetch() == capi.QUICKED_OK
    assert a.fetch() == capi.QUICKED_OK
    sa, sta = a.scores()
    sb, stb = b.scores()
    assert sa.tolist() == exp_a and sb.tolist() == exp_b
    assert (sta == capi.QUICKED_OK).all() and (stb == capi.QUICKED_OK).all()
    _check_form(a, switch, True)
    a.close()
    b.close()


def _edits(rle):
    return sum(1 for op in O.rle_to_ops(rle) if op in b"XID")


@pytest.mark.parametrize("switch", SWITCHES)
def test_cigars_of_the_pairs_within_their_bound(switch, monkeypatch):
    pairs, dist = grid()
    bounds = np.array(M.mixed_bounds(pairs), dtype=np.int32)
    exp = [M.threshold(d, k) for d, k in zip(dist, bounds)]
    _balanced(exp)
    _set_switch(monkeypatch, switch)
    rb = capi.ResidentBatch(datagen.PairBatch(*_pools(pairs)))
    assert rb.configure(cigar_style=0, check=True) == capi.QUICKED_OK
    assert rb.run_bounded(bounds, only_score=False, sync=True) == capi.QUICKED_OK
    scores, status = rb.scores()
    assert scores.tolist() == exp
    assert (status == capi.QUICKED_OK).all()
    cig, ok = rb.cigars(), rb.check_results()
    for i, (p, t) in enumerate(pairs):
        if exp[i] < 0:
            assert cig[i] is None and ok[i] == -1, i
        else:
            assert cig[i] is not None and ok[i] == 1, (i, cig[i])
            assert O.cigar_is_valid(p, t, cig[i]), (i, cig[i])
            assert _edits(cig[i]) == exp[i], (i, cig[i], exp[i])
    # the SAM styles print (checked against the style-0 string by the reference's own printers' rules)
    for style, mism in ((1, True), (2, False)):
        assert rb.configure(cigar_style=style, check=False) == capi.QUICKED_OK
        assert rb.run_bounded(bounds, only_score=False, sync=True) == capi.QUICKED_OK
        got = rb.cigars()
        for i in range(len(pairs)):
            if exp[i] < 0:
                assert got[i] is None
            else:
                assert got[i] == O.sam_cigar(cig[i], mism), (i, style, got[i], cig[i])
    rb.close()


def test_non_canonical_symbols_against_the_reference():
    pairs = M.noncanon_pairs()
    dist = M.expected("noncanon", pairs, noncanon=True)
    bounds = np.array(M.noncanon_bounds(dist), dtype=np.int32)
    exp = [M.threshold(d, k) for d, k in zip(dist, bounds)]
    _balanced(exp)
    rb = capi.ResidentBatch(datagen.PairBatch(*_pools(pairs)))
    assert rb.run_bounded(bounds) == capi.QUICKED_OK
    scores, _ = rb.scores()
    print("library:", scores.tolist())
    print("expected:", exp)
    assert scores.tolist() == exp
    # the same from a queued run, and with CIGARs: the QUICKED flow's own alignment, whose edit count is the distance
    assert rb.run_bounded(bounds, sync=False) == capi.QUICKED_OK
    assert rb.fetch() == capi.QUICKED_OK
    assert rb.scores()[0].tolist() == exp
    assert rb.run_bounded(bounds, only_score=False) == capi.QUICKED_OK
    scores, status = rb.scores()
    assert scores.tolist() == exp and (status == capi.QUICKED_OK).all()
    for i, ((p, t), c) in enumerate(zip(pairs, rb.cigars())):
        if exp[i] < 0:
            assert c is None, i
        else:
            assert c is not None and O.cigar_is_valid(p, t, c) and _edits(c) == exp[i], (i, c, exp[i])
    rb.close()


def test_other_runs_are_untouched_by_bounded_runs():
    """quicked_batch_run with BANDED / QUICKED parameters returns the same scores and CIGAR bytes before and after
    bounded runs on the same batch object, a queued one included"""
    batch = datagen.generate(count=300, length=700, error=0.04, seed=5)
    rb = capi.ResidentBatch(batch)
    other = capi.ResidentBatch(batch)

    def snapshot(obj):
        out = []
        for kw in (dict(algo=capi.BANDED, only_score=True), dict(algo=capi.BANDED), dict(algo=capi.QUICKED), dict(algo=capi.QUICKED, only_score=True)):
            st = obj.run(capi.make_params(**kw), sync=True)
            sc, stt = obj.scores()
            out.append((st, sc.tolist(), stt.tolist(), obj.cigars()))
        st = obj.run(capi.make_params(algo=capi.QUICKED), sync=False)
        assert obj.fetch() >= 0
        sc, stt = obj.scores()
        out.append((st, sc.tolist(), stt.tolist(), obj.cigars()))
        return out

    want = snapshot(other)                       # an object that never sees a bounded run
    assert snapshot(rb) == want
    assert rb.run_bounded(20) == capi.QUICKED_OK
    assert snapshot(rb) == want
    assert rb.run_bounded(30, sync=False) == capi.QUICKED_OK          # queued, then superseded by the next runs
    assert snapshot(rb) == want
    assert rb.run_bounded(25, only_score=False) == capi.QUICKED_OK
    assert rb.run_bounded(25, sync=False) == capi.QUICKED_OK
    assert rb.fetch() == capi.QUICKED_OK
    assert snapshot(rb) == want
    ms, launches = rb.kernel_times()
    rb.run(capi.make_params(algo=capi.QUICKED, only_score=True), sync=True)
    ms, launches = rb.kernel_times()
    assert launches[3] == 0                      # slot [3] stays 0 in a run that is not bounded
    rb.close()
    other.close()


def test_batch_at_size():
    """100 000 pairs of 10 kb, 0.3 % planted edits on average, bound = the median distance: against edlib on a seeded
    sample of 200 pairs, and for ALL pairs against the existing QUICKED only_score run thresholded here (a cross-check)"""
    sample = M.big_sample_indices()
    dist = M.expected("big_sample", M.big_sample_pairs())
    bound = int(np.median(dist))
    exp = [M.threshold(d, bound) for d in dist]
    _balanced(exp)
    batch = M.big_batch()
    assert len(batch) == M.BIG["count"]
    for j, i in enumerate(sample[:3]):           # the sample is the batch's own pairs
        assert (batch.pattern(i), batch.text(i)) == M.big_sample_pairs()[j]
    rb = capi.ResidentBatch(batch)
    rb.kernel_times()
    assert rb.run_bounded(bound) == capi.QUICKED_OK
    scores, status = rb.scores()
    _, launches = rb.kernel_times()
    print("bound", bound, "diagonal-word launches", int(launches[3]), "within", int((scores >= 0).sum()))
    assert [int(scores[i]) for i in sample] == exp
    assert (status == capi.QUICKED_OK).all()
    assert rb.run(capi.make_params(algo=capi.QUICKED, only_score=True), sync=True) >= 0
    full, _ = rb.scores()
    cross = np.where(full <= bound, full, -1)
    _balanced(cross)
    assert (scores == cross).all(), np.nonzero(scores != cross)[0][:10]
    rb.close()
