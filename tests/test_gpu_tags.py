"""Alignment tags on the GPU (quicked_batch_configure_tags through capi.ResidentBatch): per-pair statistics and MD:Z strings.
Expected values never come from the tag kernels: they are the definitions (tests/tags_lib.py) applied to the style-0 CIGAR
of the same run without tags and to the pair's bytes; those CIGARs are pinned to the oracle by the rest of the suite."""
import numpy as np
import pytest

import tags_lib as T
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ALGOS = {"quicked": dict(algo=capi.QUICKED), "windowed": dict(algo=capi.WINDOWED), "windowed_w2": dict(algo=capi.WINDOWED, window_size=2),
         "banded": dict(algo=capi.BANDED), "hirschberg": dict(algo=capi.HIRSCHBERG)}


def _batch(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs) or b"\0", dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1])]).astype(np.int64)
    return datagen.PairBatch(pp, po, pl, tp, to, tl)


def _run(rb, kw=None, bound=None):
    """one sync run -> (status of the call, scores, statuses, cigars)"""
    if bound is not None:
        st = rb.run_bounded(bound, only_score=False, sync=True)
    else:
        st = rb.run(capi.make_params(**kw), sync=True)
    assert st >= 0 or st == capi.QUICKED_EMPTY_SEQUENCE, st
    sc, stt = rb.scores()
    return st, sc, stt, rb.cigars()


def _forced_run(rb, tw, kw=None, bound=None):
    """_run with QE_TAGS_WAVE = tw in force: every count pass the run launched must have been of that form (the library's
    process-wide launch counts, lane form / wave form)"""
    before = capi.tag_launches()
    out = _run(rb, kw, bound)
    after = capi.tag_launches()
    other, forced = (0, 1) if tw == "1" else (1, 0)
    assert after[forced] > before[forced] and after[other] == before[other], (tw, before, after)
    return out


def _check_tags(pairs, rb, base, expected, md=True, label=None):
    """the run that just ended against the tags-0 run `base` = (st, scores, statuses, cigars) of the same configuration and
    `expected` = tags_lib.expected_from_cigars of the style-0 CIGARs"""
    sc, stt = rb.scores()
    assert (sc == base[1]).all() and (stt == base[2]).all(), label
    stats = rb.pair_stats()
    mds = rb.md() if md else None
    for i, (p, t) in enumerate(pairs):
        want_stats, want_md = expected[i]
        assert tuple(int(x) for x in stats[i]) == want_stats, (label, i, len(p), len(t), stats[i], want_stats)
        if md:
            assert mds[i] == want_md, (label, i, len(p), len(t), mds[i], want_md)
        if want_md is not None:
            assert T.identities_hold(want_stats, len(p), len(t), int(sc[i])), (label, i)
    if md:
        # offsets: how the strings lie in the pool is the library's business; they must be disjoint and inside it
        nb = rb._lib.quicked_batch_md_bytes(rb._h)
        off = np.zeros(rb.n, dtype=np.int64)
        assert rb._lib.quicked_batch_md(rb._h, None, off.ctypes.data) == capi.QUICKED_OK
        spans = sorted((int(o), int(o) + len(m) + 1) for o, m in zip(off, mds) if m is not None)
        assert all(o == -1 for o, m in zip(off, mds) if m is None)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or (spans[0][0] >= 0 and spans[-1][1] <= nb))


def ragged_pairs():
    """every combination of the lengths at 10 % error, then ragged pairs with empty sequences, N, lower case and IUPAC"""
    rng = np.random.default_rng(8101)
    lens = (1, 2, 63, 64, 65, 130, 300)
    pairs = []
    for m in lens:
        for n in lens:
            p = T.random_seq(rng, m)
            t = T.mutate(rng, p, 0.10)
            t = (t + T.random_seq(rng, n))[:n]
            pairs.append((p, t))
    for i in range(24):
        p = T.random_seq(rng, 20 + 27 * i)
        t = T.mutate(rng, p, 0.08)
        p, t = bytearray(p), bytearray(t)
        if i % 4 == 1:
            for k in rng.integers(0, len(p), 3): p[k] = ord("N")
            for k in rng.integers(0, len(t), 3): t[k] = ord("N")
        if i % 4 == 2:
            p = bytearray(bytes(p).lower())
        if i % 4 == 3:
            for k in rng.integers(0, len(t), 2): t[k] = ord("R")
            for k in rng.integers(0, len(p), 2): p[k] = ord("n")
        pairs.append((bytes(p), bytes(t)))
    pairs[50] = (b"", pairs[50][1])
    pairs[52] = (pairs[52][0], b"")
    pairs[54] = (b"", b"")
    return pairs


@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_ragged_small_pairs_every_form_layout_and_style(algo, monkeypatch):
    pairs = ragged_pairs()
    kw = ALGOS[algo]
    rb = capi.ResidentBatch(_batch(pairs))
    for fw in ("0", "1"):
        monkeypatch.setenv("QE_FORMAT_WAVE", fw)
        assert rb.configure(0) == 0 and rb.configure_tags() == 0
        expected = T.expected_from_cigars(pairs, _run(rb, kw)[3])
        assert sum(1 for _, m in expected if m is not None) >= len(pairs) - 3 - (20 if algo == "banded" else 0)
        for style in (0, 1, 2):
            assert rb.configure(style) == 0 and rb.configure_tags() == 0
            base = _run(rb, kw)
            for tw in ("0", "1"):
                monkeypatch.setenv("QE_TAGS_WAVE", tw)
                assert rb.configure_tags(stats=True, md=True) == 0
                got = _forced_run(rb, tw, kw)
                assert got[0] == base[0] and got[3] == base[3], (algo, fw, style, tw)
                _check_tags(pairs, rb, base, expected, label=(algo, fw, style, tw))
    rb.close()


@pytest.mark.parametrize("algo", ["hirschberg", "quicked"])
def test_segment_borders_and_the_carry_between_wave_steps(algo, monkeypatch):
    """150 pairs of 1 200 at 10 % with QE_SPLIT_BYTES=4096: many leaves per alignment, equal runs meeting at their borders.
    Alignments of 1 200 bases at 10 % have 190-230 runs, four wave steps; ten pairs of 500 (85-95 runs) ride along so that
    the batch also has alignments of exactly two steps"""
    monkeypatch.setenv("QE_SPLIT_BYTES", "4096")
    pairs = list(datagen.generate(count=150, length=1200, error=0.10, seed=7001).pairs()) + \
        list(datagen.generate(count=10, length=500, error=0.10, seed=7101).pairs())
    rb = capi.ResidentBatch(_batch(pairs))
    base = _run(rb, ALGOS[algo])
    assert all(c is not None for c in base[3])
    nruns = [T.n_runs(c) for c in base[3]]
    assert any(x > 128 for x in nruns) and any(65 <= x <= 128 for x in nruns), (min(nruns), max(nruns))
    expected = T.expected_from_cigars(pairs, base[3])
    for tw in ("0", "1"):
        monkeypatch.setenv("QE_TAGS_WAVE", tw)
        assert rb.configure_tags(stats=True, md=True) == 0
        got = _forced_run(rb, tw, ALGOS[algo])
        assert got[3] == base[3]
        _check_tags(pairs, rb, base, expected, label=(algo, tw))
    rb.close()


def long_run_pairs():
    rng = np.random.default_rng(8201)
    out = []
    s = T.random_seq(rng, 5000)
    flip = bytes([b"ACGT"[(b"ACGT".index(s[2500]) + 1) % 4]])
    out.append((s, s[:2500] + flip + s[2501:]))                       # one mismatch in the middle
    out.append((s, s[:2500] + s[2503:]))                              # one 3-base deletion (D consumes pattern)
    out.append((s, s[:2400] + s[2470:]))                              # one 70-base deletion
    flip = bytes([b"ACGT"[(b"ACGT".index(s[3003]) + 2) % 4]])
    out.append((s, s[:3000] + flip + s[3004:]))                       # a mismatch directly after a deletion
    return out


def test_long_match_runs_across_wave_steps_and_four_digit_numbers(monkeypatch):
    pairs = long_run_pairs()
    rb = capi.ResidentBatch(_batch(pairs))
    base = _run(rb, ALGOS["quicked"])
    expected = T.expected_from_cigars(pairs, base[3])
    assert expected[0][0][6] >= 2499 and expected[2][0][3] == 70 and any(m and "^" in m for _, m in expected)
    assert all(any(len(w) >= 4 for w in "".join(ch if ch.isdigit() else " " for ch in m).split()) for _, m in expected)
    for tw in ("0", "1"):
        monkeypatch.setenv("QE_TAGS_WAVE", tw)
        for fw in ("0", "1"):
            monkeypatch.setenv("QE_FORMAT_WAVE", fw)
            assert rb.configure_tags(stats=True, md=True) == 0
            got = _forced_run(rb, tw, ALGOS["quicked"])
            assert got[3] == base[3]
            _check_tags(pairs, rb, base, expected, label=(tw, fw))
    rb.close()


def test_long_reads_in_the_form_the_library_picks(monkeypatch):
    monkeypatch.delenv("QE_TAGS_WAVE", raising=False)
    monkeypatch.delenv("QE_FORMAT_WAVE", raising=False)
    pairs = list(datagen.generate(count=4, length=100_000, error=0.10, seed=8301).pairs())
    rb = capi.ResidentBatch(_batch(pairs))
    base = _run(rb, ALGOS["quicked"])
    assert all(c is not None for c in base[3])
    expected = T.expected_from_cigars(pairs, base[3])
    assert rb.configure_tags(stats=True, md=True) == 0
    got = _forced_run(rb, "1", ALGOS["quicked"])                     # unforced: 30 k runs per pair go to the wave form
    assert got[3] == base[3]
    _check_tags(pairs, rb, base, expected)
    # ... and so do they without the strings: the run is laid out as the CIGAR run of the same pairs
    assert rb.configure_tags(stats=True, cigar=False) == 0
    got = _forced_run(rb, "1", ALGOS["quicked"])
    assert all(c is None for c in got[3])
    _check_tags(pairs, rb, base, expected, md=False)
    rb.close()


@pytest.mark.parametrize("algo", ["quicked", "hirschberg", "windowed"])
def test_no_cigar_keeps_scores_statuses_and_stats(algo):
    pairs = ragged_pairs()
    rb = capi.ResidentBatch(_batch(pairs))
    assert rb.configure(0, check=True) == 0
    base = _run(rb, ALGOS[algo])
    assert (rb.check_results()[[i for i, c in enumerate(base[3]) if c is not None]] == 1).all()
    expected = T.expected_from_cigars(pairs, base[3])
    assert rb.configure_tags(stats=True, cigar=False) == 0
    got = _run(rb, ALGOS[algo])
    assert got[0] == base[0] and all(c is None for c in got[3])
    assert rb._lib.quicked_batch_cigar_bytes(rb._h) == 0
    off = np.zeros(rb.n, dtype=np.int64)
    rb._lib.quicked_batch_cigars(rb._h, None, off.ctypes.data)
    assert (off == -1).all() and (rb.check_results() == -1).all()
    _check_tags(pairs, rb, base, expected, md=False, label=algo)
    with pytest.raises(capi.QuickedException):
        rb.md()                                                      # STATS | NO_CIGAR produces no MD data
    rb.close()


def test_bounded_runs_carry_tags_for_the_pairs_within_their_bound(monkeypatch):
    pairs = [p for p in ragged_pairs() if len(p[0]) and len(p[1])]
    rb = capi.ResidentBatch(_batch(pairs))
    bound = 12
    base = _run(rb, bound=bound)
    within = [c is not None for c in base[3]]
    assert sum(within) * 5 >= len(pairs) and (len(pairs) - sum(within)) * 5 >= len(pairs)
    assert all((c is not None) == (0 <= s <= bound) for c, s in zip(base[3], base[1]))
    expected = T.expected_from_cigars(pairs, base[3])
    for tw in ("0", "1"):
        monkeypatch.setenv("QE_TAGS_WAVE", tw)
        assert rb.configure_tags(stats=True, md=True) == 0
        got = _forced_run(rb, tw, bound=bound)
        assert got[3] == base[3]
        _check_tags(pairs, rb, base, expected, label=tw)
        assert rb.configure_tags(stats=True, md=True, cigar=False) == 0
        got = _run(rb, bound=bound)
        assert all(c is None for c in got[3])
        _check_tags(pairs, rb, base, expected, label=(tw, "no cigar"))
    rb.close()


def test_packed_batches_take_stats_and_refuse_md():
    pairs = [p for p in ragged_pairs()[:49] if len(p[0]) and len(p[1])]
    batch = _batch(pairs)
    rb = capi.ResidentBatch(batch)
    base = _run(rb, ALGOS["quicked"])
    expected = T.expected_from_cigars(pairs, base[3])
    rb.close()
    for wire in (capi.WIRE_2BIT, capi.WIRE_PLANES3):
        rbp = capi.ResidentBatch(batch, wire=wire)
        assert rbp.configure_tags(md=True) == capi.QUICKED_UNIMPLEMENTED
        assert rbp.configure_tags(stats=True, md=True) == capi.QUICKED_UNIMPLEMENTED
        assert rbp.configure_tags(stats=True) == capi.QUICKED_OK
        got = _run(rbp, ALGOS["quicked"])
        assert got[3] == base[3]
        _check_tags(pairs, rbp, base, expected, md=False, label=wire)
        assert rbp.configure_tags(stats=True, cigar=False) == capi.QUICKED_OK
        got = _run(rbp, ALGOS["quicked"])
        assert all(c is None for c in got[3])
        _check_tags(pairs, rbp, base, expected, md=False, label=(wire, "no cigar"))
        rbp.close()


def test_surface_rules():
    pairs = list(datagen.generate(count=70, length=300, error=0.08, seed=8401).pairs())
    rb = capi.ResidentBatch(_batch(pairs))
    lib, h = rb._lib, rb._h
    assert lib.quicked_batch_configure_tags(h, 8) == capi.QUICKED_ERROR and lib.quicked_batch_configure_tags(h, -1) == capi.QUICKED_ERROR
    stats = np.zeros((rb.n, 8), dtype=np.int32)
    off = np.zeros(rb.n, dtype=np.int64)

    def getters():
        return lib.quicked_batch_pair_stats(h, stats.ctypes.data), lib.quicked_batch_md(h, None, off.ctypes.data), lib.quicked_batch_md_bytes(h)

    p = capi.make_params(algo=capi.QUICKED)
    ps = capi.make_params(algo=capi.QUICKED, only_score=True)
    # tags 0: today's behaviour, and the getters have nothing
    base = _run(rb, dict(algo=capi.QUICKED))
    assert getters() == (capi.QUICKED_ERROR, capi.QUICKED_ERROR, 0)
    expected = T.expected_from_cigars(pairs, base[3])
    assert rb.configure_tags(stats=True, md=True) == 0
    # a queued run that aligns cannot carry tags: nothing is queued, the results of the last run stay
    assert rb.run(p, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert rb.fetch() == capi.QUICKED_OK and rb.cigars() == base[3]
    # a queued only_score run ignores them
    assert rb.run(ps, sync=False) >= 0 and rb.fetch() == capi.QUICKED_OK
    assert (rb.scores()[0] == base[1]).all() and getters() == (capi.QUICKED_ERROR, capi.QUICKED_ERROR, 0)
    # a sync run with tags, then an only_score sync run: no tag data again
    got = _run(rb, dict(algo=capi.QUICKED))
    assert got[3] == base[3]
    _check_tags(pairs, rb, base, expected)
    assert rb.run(ps, sync=True) >= 0
    assert getters() == (capi.QUICKED_ERROR, capi.QUICKED_ERROR, 0)
    # configure_tags(0) restores today's behaviour: a queued run plus fetch works, and a sync run leaves no tag data
    assert rb.configure_tags() == 0
    assert rb.run(p, sync=False) >= 0 and rb.fetch() == capi.QUICKED_OK
    sc, stt = rb.scores()
    assert (sc == base[1]).all() and (stt == base[2]).all() and rb.cigars() == base[3]
    assert getters() == (capi.QUICKED_ERROR, capi.QUICKED_ERROR, 0)
    got = _run(rb, dict(algo=capi.QUICKED))
    assert got[3] == base[3] and getters() == (capi.QUICKED_ERROR, capi.QUICKED_ERROR, 0)
    rb.close()
