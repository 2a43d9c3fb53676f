"""Panel search on the GPU (quicked_batch_run_panel through capi.ResidentBatch.run_panel): every text of a batch against one
shared set of patterns.  Expected values never come from the library: tests/panel_lib.py -- the per-pair brute forces and the
key order -- over the matrices recorded in tests/golden/search_panel_cases.json (a sample of which
tests/test_search_panel_cpu.py recomputes), or computed live for the small sets made here.  The one test at size compares the
library's two routes with each other (the panel run against the n x K pair batch through run_search, reduced in numpy by the
key order) and a fixed sample of its texts with panel_lib."""
import importlib.util
import os

import numpy as np
import pytest

import panel_lib as P
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX, INFIX = capi.SEARCH_PREFIX, capi.SEARCH_INFIX
MODES = [PREFIX, INFIX]
FLAGS = [0, capi.SEARCH_IUPAC, capi.SEARCH_IUPAC_PATTERN]
SLICES = [None, "1", "2", "4096"]                 # QE_PANEL_SLICES: the host's choice, one, two, one per member
INT_MAX = 2**31 - 1
ACGT = b"ACGT"


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_search_panel_cases")


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


def got_hits(rb):
    r = rb.panel_results()
    return np.stack([r[f] for f in P.HIT_FIELDS], axis=1).astype(np.int64)


def run_and_compare(rb, texts, panel, mode, flag, bounds, matrix, D=None, E=None):
    """bounds: one int (through max_dist_all) or one per member; every field of every text, the statuses, the scores getter,
    the other getters' refusals and -- matrix -- every {d, text_end}"""
    per_member = [int(bounds)] * len(panel) if np.ndim(bounds) == 0 else [int(b) for b in bounds]
    hits, Db, Eb = P.expected(texts, panel, per_member, mode, flag, D, E)
    arg = int(bounds) if np.ndim(bounds) == 0 else np.asarray(bounds, dtype=np.int32)
    assert rb.run_panel(mode | flag, panel, arg, matrix=matrix) == capi.QUICKED_OK
    got = got_hits(rb)
    bad = [(i, len(texts[i]), got[i].tolist(), hits[i].tolist()) for i in range(len(texts)) if got[i].tolist() != hits[i].tolist()]
    assert not bad, (mode, flag, len(bad), bad[:6])
    sc, st = rb.scores()
    assert sc.tolist() == hits[:, 1].tolist()
    assert st.tolist() == [capi.QUICKED_OK if t else capi.QUICKED_EMPTY_SEQUENCE for t in texts]
    assert all(c is None for c in rb.cigars())
    with pytest.raises(capi.QuickedException):
        rb.locations()
    with pytest.raises(capi.QuickedException):
        rb.hits()
    if matrix:
        ms, me = rb.panel_matrix()
        assert ms.shape == (len(texts), len(panel))
        assert np.array_equal(ms, Db) and np.array_equal(me, Eb), (mode, flag, np.argwhere(ms != Db)[:6].tolist(), np.argwhere(me != Eb)[:6].tolist())
    else:
        with pytest.raises(capi.QuickedException):
            rb.panel_matrix()
    return hits


@pytest.mark.parametrize("nslices", SLICES)
@pytest.mark.parametrize("name", ["named", "random"])
def test_named_and_random_sets(sets, name, nslices, monkeypatch):
    s = sets[name]
    texts, panel = s["texts"], s["panel"]
    slices(monkeypatch, nslices)
    rb = batch_of(texts)
    for mode in MODES:
        for flag in FLAGS:
            D, E = s["matrix"][(mode, flag)]
            rb.kernel_times()
            hits = run_and_compare(rb, texts, panel, mode, flag, s["bounds"], True, D, E)
            _, launches = rb.kernel_times()
            assert launches[0] >= (2 if mode == INFIX else 1) and rb.counters()[0] > 0      # the passes: slot [0] of both
            assert any(h[4] >= 0 for h in hits)
            hits = run_and_compare(rb, texts, panel, mode, flag, s["uniform"], False, D, E)
            # (a member whose own bound is INT32_MAX is within it in every text; under the uniform bound some texts have none)
            assert any(h[0] < 0 for h in hits) and any(h[0] >= 0 for h in hits)
    rb.close()


def _rand(rng, n):
    return bytes(ACGT[int(x)] for x in rng.integers(0, 4, n))


def small_set(n, k, seed):
    """n texts of 20 .. 140 bases, each holding one of k members of 12 .. 80 bases with a few errors"""
    rng = np.random.default_rng(seed)
    panel = [_rand(rng, int(rng.integers(12, 81))) for _ in range(k)]
    texts = [G.plant(rng, int(rng.integers(20, 141)), [G.mutate(rng, panel[int(rng.integers(0, k))], 0.06)]) for _ in range(n)]
    return texts, panel


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_partial_waves(n, monkeypatch):
    texts, panel = small_set(n, 5, 100 + n)
    rb = batch_of(texts)
    for nslices in (None, "2"):
        slices(monkeypatch, nslices)
        for mode in MODES:
            run_and_compare(rb, texts, panel, mode, 0, 6, True)
    rb.close()


@pytest.mark.parametrize("k", [1, 2, 3, 64, 65])
def test_panel_sizes(k, monkeypatch):
    texts, panel = small_set(24, k, 200 + k)
    D, E = P.matrix(texts, panel, INFIX, 0)
    rb = batch_of(texts)
    for nslices in SLICES:
        slices(monkeypatch, nslices)
        hits = run_and_compare(rb, texts, panel, INFIX, 0, 8, True, D, E)
        assert k > 1 or all(h[4] < 0 for h in hits)              # one member: never a runner-up
    rb.close()


def test_the_batch_patterns_play_no_part(sets):
    s = sets["named"]
    texts, panel = s["texts"], s["panel"]
    rng = np.random.default_rng(9)
    long_patterns = [_rand(rng, 700 - 13 * (i % 40)) for i in range(len(texts))]
    out = []
    for patterns in (None, long_patterns):
        rb = batch_of(texts, patterns)
        assert rb.run_panel(INFIX, panel, s["bounds"], matrix=True) == capi.QUICKED_OK
        out.append((got_hits(rb), rb.scores(), rb.panel_matrix()))
        rb.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1][0], out[1][1][0]) and np.array_equal(out[0][1][1], out[1][1][1])
    assert np.array_equal(out[0][2][0], out[1][2][0]) and np.array_equal(out[0][2][1], out[1][2][1])
    hits, _, _ = P.expected(texts, panel, s["bounds"], INFIX, 0, *s["matrix"][(INFIX, 0)])
    assert np.array_equal(out[1][0], hits)


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
            res = []
            for rb in (rp, ra):
                assert rb.run_panel(mode | flag, s["panel"], s["bounds"], matrix=True) == capi.QUICKED_OK
                res.append((got_hits(rb), rb.panel_matrix()))
            assert np.array_equal(res[0][0], res[1][0]), (mode, flag)
            assert np.array_equal(res[0][1][0], res[1][1][0]) and np.array_equal(res[0][1][1], res[1][1][1])
            D, E = s["matrix"][(mode, flag)]
            hits, _, _ = P.expected(texts, s["panel"], s["bounds"], mode, flag, D[keep], E[keep])
            assert np.array_equal(res[0][0], hits), (mode, flag)
    rp.close()
    ra.close()


def reduce_pairs(sc, ts, te, n, k):
    """the n x K pair batch's answers ([text][member]) reduced by the key order -> hits [n][6]"""
    sc, ts, te = sc.reshape(n, k).astype(np.int64), ts.reshape(n, k), te.reshape(n, k)
    key = np.where(sc >= 0, sc * (k + 1) + np.arange(k)[None, :], np.iinfo(np.int64).max)
    order = np.argsort(key, axis=1, kind="stable")
    rows = np.arange(n)
    b, r = order[:, 0], order[:, 1] if k > 1 else order[:, 0]
    has1 = sc[rows, b] >= 0
    has2 = (sc[rows, r] >= 0) & (k > 1)
    out = np.full((n, 6), -1, dtype=np.int64)
    out[has1, 0] = b[has1]; out[has1, 1] = sc[rows, b][has1]; out[has1, 2] = ts[rows, b][has1]; out[has1, 3] = te[rows, b][has1]
    out[has2, 4] = r[has2]; out[has2, 5] = sc[rows, r][has2]
    return out


def test_route_agreement_at_size():
    """20 000 texts of 150 bases x 48 members of 20 .. 40 bases: the panel run against the library's pairwise route"""
    rng = np.random.default_rng(77)
    n, k = 20000, 48
    panel = [_rand(rng, int(rng.integers(20, 41))) for _ in range(k)]
    panel[5] = panel[4]                                            # a duplicate, and a near-duplicate
    panel[7] = panel[6][:9] + bytes([ACGT[(ACGT.index(panel[6][9]) + 1) % 4]]) + panel[6][10:]
    codes = rng.integers(0, 4, (n, 150)).astype(np.uint8)
    tarr = np.frombuffer(ACGT, dtype=np.uint8)[codes]
    which = rng.integers(0, k, n)
    for i in range(n):
        q = G.mutate(rng, panel[int(which[i])], 0.08) if i % 10 else b""      # every tenth text holds nothing
        at = int(rng.integers(0, 150 - len(q) + 1))
        tarr[i, at:at + len(q)] = np.frombuffer(q, dtype=np.uint8)
    texts = [tarr[i].tobytes() for i in range(n)]
    bound = 5
    rb = batch_of(texts)
    assert rb.run_panel(INFIX, panel, bound) == capi.QUICKED_OK
    got = got_hits(rb)
    rb.close()
    # the pairwise route: pair i * K + p is member p against text i
    pp, po, pl = _pool(panel * n)
    tp = np.repeat(tarr, k, axis=0).reshape(-1)
    tl = np.full(n * k, 150, dtype=np.int32)
    to = (np.arange(n * k, dtype=np.int64) * 150)
    rq = capi.ResidentBatch(datagen.PairBatch(pp, po, pl, tp, to, tl))
    assert rq.run_search(INFIX, bound, only_score=True) == capi.QUICKED_OK
    sc, _ = rq.scores()
    ts, te = rq.locations()
    rq.close()
    want = reduce_pairs(sc, ts, te, n, k)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]])
    assert int((got[:, 0] >= 0).sum()) > n // 2 and int((got[:, 0] < 0).sum()) > n // 50 and int((got[:, 4] >= 0).sum()) > 100
    sample = [int(i) for i in np.random.default_rng(3).choice(n, 200, replace=False)]
    hits, _, _ = P.expected([texts[i] for i in sample], panel, [bound] * k, INFIX, 0)
    assert np.array_equal(got[sample], hits)


def test_panel_and_search_runs_in_turn(sets):
    s = sets["named"]
    texts, panel = s["texts"], s["panel"]
    patterns = [panel[i % len(panel)] for i in range(len(texts))]
    rb = batch_of(texts, patterns)
    with pytest.raises(capi.QuickedException):
        rb.panel_results()
    for _ in range(2):
        run_and_compare(rb, texts, panel, INFIX, 0, s["bounds"], True, *s["matrix"][(INFIX, 0)])
        assert rb.run_search(INFIX, 10, only_score=True) == capi.QUICKED_OK
        ts, te = rb.locations()
        sc, st = rb.scores()
        for i, (q, t) in enumerate(zip(patterns, texts)):
            if not t:
                assert st[i] == capi.QUICKED_EMPTY_SEQUENCE
                continue
            d, e = P.pair_answer(q, t, INFIX, 0)
            assert (int(sc[i]), int(te[i])) == ((d, e) if d <= min(10, len(q)) else (-1, -1)), i
        with pytest.raises(capi.QuickedException):
            rb.panel_results()
        with pytest.raises(capi.QuickedException):
            rb.panel_matrix()
    rb.close()


def test_argument_rules_on_the_device(sets):
    s = sets["named"]
    rb = batch_of(s["texts"][:8])
    panel = s["panel"]
    assert rb.run_panel(INFIX, panel, 3) == capi.QUICKED_OK
    before = got_hits(rb)
    cnt = rb.counters()[0]
    assert rb.run_panel(INFIX | capi.SEARCH_IUPAC | capi.SEARCH_IUPAC_PATTERN, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel(3, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX | 128, panel, 3) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX, panel + [b""], 3) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX, panel, -1) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX, [b"ACGT"] * 4097, 3) == capi.QUICKED_ERROR
    assert rb.run_panel(INFIX, panel + [b"A" * 257], 3) == capi.QUICKED_UNIMPLEMENTED
    assert rb.run_panel(INFIX, panel, 3, sync=False) == capi.QUICKED_UNIMPLEMENTED
    assert np.array_equal(got_hits(rb), before) and rb.counters()[0] == cnt      # nothing ran
    rb.close()
