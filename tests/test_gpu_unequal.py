"""Pairs of unequal lengths on the GPU: the 144 pairs of tests/unequal_lib.py (texts from half to twice their pattern, the
surplus cut from the end or out of the middle) in one batch, through the library's own selection and through every forced
kernel form, against the oracle -- which tests/test_oracle_vs_ref.py pins to the compiled reference on these very pairs.
The length difference is an input of the band geometry every form restates (prologue, relative cutoff, effective
bandwidth, the last block's place in the band); datagen's pairs keep it at a few values.

The domain rule is unequal_lib.in_domain, the CPU half's: CIGAR-producing BandEd / Hirschberg are compared where the
distance is within the cutoff, score-only BandEd on all 144 pairs (the -1 of a band below the distance is this library's
definition, DESIGN.md 5: the GPU has to give exactly it), everything else on all 144."""
import ctypes as C
import functools
import re
import shutil

import pytest

import masked_lib as ML
import narrow_fit_lib as FL
import narrow_lib as NL
import narrow_prune_lib as PL
import oracle_lib as O
import tags_lib as T
import unequal_lib as U
from quicked_amd import capi, datagen
from test_gpu_parity import _pools, exact_cached, gpu_batch, oracle_cached

pytestmark = pytest.mark.gpu

SCORE_SETS = ("banded_so_bw15", "banded_so_bw40")
FILL_SETS = ("banded_bw40", "quicked")
WINDOWED_SETS = ("windowed_so", "windowed", "windowed_w2", "windowed_w2_scalar")
CAP = 13            # qe_types.h: score_lds_cap()


def ident(env):
    return "-".join(f"{k[3:]}={v}" for k, v in env.items()) or "default"


@functools.lru_cache(maxsize=None)
def pairs():
    return tuple(U.pairs())


def batch_of(prs):
    return datagen.PairBatch(*_pools(list(prs)))


@functools.lru_cache(maxsize=None)
def expected(name, **more):
    """-> per pair (status, score, cigar, trace) of the oracle and whether the pair is inside the domain -- computed once,
    shared by the tests, never changed"""
    kw = dict(U.PARAM_SETS[name], **more)
    exp = [oracle_cached(p, t, trace=True, **kw) for p, t in pairs()]
    dom = [U.in_domain(kw, len(p), len(t), exact_cached(p, t), e[1]) for (p, t), e in zip(pairs(), exp)]
    return kw, exp, dom


def compare(name, status, scores, cig, label, **more):
    """-> the number of pairs compared"""
    kw, exp, dom = expected(name, **more)
    everywhere = kw["algo"] == U.BANDED and kw.get("only_score")
    n = 0
    for i, (p, t) in enumerate(pairs()):
        if not (everywhere or dom[i]):
            continue
        where = (name, label, i + 1, len(p), len(t))
        assert (int(status[i]), int(scores[i])) == exp[i][:2], where
        if cig is not None:
            assert cig[i] == exp[i][2], where
        n += 1
    assert n >= U.MIN_INSIDE[name], (name, n)
    return n


def work_of(name, key, **more):
    return sum(e[3][key] for e in expected(name, **more)[1])


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the library's own selection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.PARAM_SETS))
def test_own_selection_resident_batch(name):
    kw = U.PARAM_SETS[name]
    scores, status, cig, cnt = gpu_batch(batch_of(pairs()), **kw)
    n = compare(name, status, scores, cig, "resident")
    print(name, "compared", n, "of", len(pairs()), "counters", [int(c) for c in cnt[:8]])
    if kw["algo"] == U.BANDED and kw.get("only_score"):
        assert cnt[0] == work_of(name, "score_block_advances"), name
    if name.startswith("banded_bw") or name.startswith("quicked"):
        assert cnt[1] == work_of(name, "fill_block_advances"), name


@pytest.mark.parametrize("name", ["quicked", "banded_bw40"])
def test_own_selection_per_pair_path(name):
    kw, exp, dom = expected(name)
    al = capi.QuickedAligner()
    for k, v in kw.items():
        setattr(al._params, k, v)
    st, out = al.alignBatch(list(pairs()))
    compare(name, [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], "alignBatch")


# ---------------------------------------------------------------------------------------------------------------------
# (b) forced forms: BandEd score-only
# ---------------------------------------------------------------------------------------------------------------------
SCORE_FORMS = [{"QE_LANE_REL": "0"}, {"QE_LANE_REL": "1"}, {"QE_SCORE_SYS": "1"}, {"QE_SCORE_SYS": "0"}, {"QE_WAVE": "1"}] + \
              [{"QE_COOP_G": g, "QE_COOP_LDS": lds} for g in ("2", "4", "8", "16", "32") for lds in ("1", "0")]


@pytest.mark.parametrize("env", SCORE_FORMS, ids=ident)
@pytest.mark.parametrize("name", SCORE_SETS)
def test_score_only_forms(name, env, monkeypatch):
    setenv(monkeypatch, env)
    scores, status, _, cnt = gpu_batch(batch_of(pairs()), **U.PARAM_SETS[name])
    compare(name, status, scores, None, ident(env))
    assert cnt[0] == work_of(name, "score_block_advances"), (name, env, int(cnt[6]))


# the two-pass path.  A first launch lays every group out like the neediest one, and a list whose uniform workspace is more
# than twice its own keeps the single pass (qe_stages.hip: run_banded_score), as does one whose band state is past the LDS
# slice: so the grid also runs in its three thirds (cases 1-48, 49-96, 97-144: one group of 64 each, whose uniform layout
# is its own) and in those pairs of the last third whose first launch fits the slice (again one group).  The patterns of the
# first two thirds are 200 bases at the most: every cutoff is the floor's, no band is narrower at half of it, and a run
# over them has no first launch.  The library's QE_TRACE line says which launch a run took.
def _fits_lds(bandwidth):
    return [i for i, (p, t) in enumerate(pairs()) if i >= 96 and
            NL.slots(len(p), len(t), NL.narrow_cutoff(len(p), len(t), NL.max_cutoff(len(p), len(t), bandwidth))) <= CAP]


def narrow_lists(bandwidth):
    n = len(pairs())
    return {"all": list(range(n)), "third_1": list(range(0, 48)), "third_2": list(range(48, 96)), "third_3": list(range(96, n)),
            "lds": _fits_lds(bandwidth)}


NARROW_FORMS = {
    "half": lambda k: {"QE_NARROW_FIT": "0", "QE_NARROW_PRUNE": "0"},
    "fit": lambda k: {"QE_NARROW_FIT": str(k), "QE_NARROW_PRUNE": "0"},
    "fit_prune": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k)),
    "unmasked": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k), QE_SCORE_MASKED="0"),
    "masked": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k), QE_SCORE_MASKED="1"),
    "lds_off": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k), QE_SCORE_LDS="0"),
    "lds_tall": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k), QE_SCORE_LDS="1", QE_SCORE_TALL="1"),
    "lds_no_tall": lambda k: dict(ML.ONE_LANE, QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(k), QE_SCORE_LDS="1", QE_SCORE_TALL="0"),
}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    d = str(tmp_path_factory.mktemp("unequal"))
    return d, PL.build_walk(d)


FORCED_K = 400      # the ratio where a run at C / 2 over the list reports none (nothing it lowered was accepted): 0.39 C


@functools.lru_cache(maxsize=None)
def narrow_model(bandwidth, which, form, work):
    """-> the list's pairs, the ratio k its forms are fitted and pruned to (what a run at C / 2 over it reports, or FORCED_K), the model's
    (scores, counters[0], counters[7]) of the two-pass run and of the single pass -- computed once, shared, never changed"""
    prs = [pairs()[i] for i in narrow_lists(bandwidth)[which]]
    memo = {}
    half = FL.fit_model(prs, 0, bandwidth=bandwidth, memo=memo)
    k = FL.learned_q(half) or FORCED_K
    if form == "half":
        model = half
    elif form == "fit":
        model = FL.fit_model(prs, k, bandwidth=bandwidth, memo=memo)
    else:
        d, exe = work
        model, _ = PL.prune_model(prs, k, k, exe, d, bandwidth=bandwidth, memo=memo, name=f"unequal_{bandwidth}_{which}")
    single = ([r["score"] for r in half], sum(r["adv"] for r in half), 0)
    return prs, k, FL.totals(model), single


@pytest.mark.parametrize("form", list(NARROW_FORMS))
@pytest.mark.parametrize("which", ["all", "third_1", "third_2", "third_3", "lds"])
@pytest.mark.parametrize("name", SCORE_SETS)
def test_score_only_two_passes(name, which, form, work, monkeypatch, capfd):
    kw = U.PARAM_SETS[name]
    prs, k, two, single = narrow_model(kw["bandwidth"], which, form, work)
    want = [oracle_cached(p, t, **kw)[:2] for p, t in prs]
    assert [w[1] for w in want] == single[0]                     # the model's single pass is the oracle's result
    setenv(monkeypatch, dict(NARROW_FORMS[form](k), QE_SCORE_NARROW="1", QE_TRACE="1"))
    rb = capi.ResidentBatch(batch_of(prs))
    try:
        for sync in (True, False):
            capfd.readouterr()
            assert rb.run(capi.make_params(**kw), sync=sync) >= 0
            if not sync:
                assert rb.fetch() >= 0
            err = capfd.readouterr().err
            launch = re.findall(r"first launch of (\d+) groups, band state in (LDS|the group workspace) \((\d+) slots\), tall passes (on|off)", err)
            scores, status = rb.scores()
            cnt = rb.counters()
            with capfd.disabled():
                print(name, which, form, "sync" if sync else "queued", "k", k, "pairs", len(prs), "first launch", launch,
                      "adv / second-pass tasks", (int(cnt[0]), int(cnt[7])), "two passes", two[1:], "single", single[1:])
            assert [(int(a), int(b)) for a, b in zip(status, scores)] == want, (name, which, form, sync)
            assert len(launch) == (1 if which in ("third_3", "lds") else 0), (name, which, form, launch)
            assert (int(cnt[0]), int(cnt[7])) == (two[1:] if launch else single[1:]), (name, which, form, sync, launch)
            if which == "lds" and form.startswith("lds_") and form != "lds_off":
                assert launch[0][1] == "LDS" and 3 <= int(launch[0][2]) <= CAP, launch
                assert launch[0][3] == ("on" if form == "lds_tall" else "off"), launch
            if which == "third_3" or form == "lds_off":
                assert launch == [] or launch[0][1:3] == ("the group workspace", "0"), launch     # (third_3: bands past the slice)
    finally:
        rb.close()


# ---------------------------------------------------------------------------------------------------------------------
# (b) forced forms: the fill and what follows it
# ---------------------------------------------------------------------------------------------------------------------
FILL_FORMS = [{"QE_FILL_MULTI": "1"}, {"QE_FILL_MULTI": "0"}, {"QE_FILL_SYS": "1"}, {"QE_FILL_SYS": "0"},
              {"QE_COOP_FILL_G": "2"}, {"QE_COOP_FILL_G": "4"}, {"QE_COOP_FILL_G": "8"},
              {"QE_COOP_TALL_FILL": "1"}, {"QE_COOP_TALL_FILL": "0"},
              {"QE_TRACE_SYS": "1"}, {"QE_TRACE_SYS": "8"}, {"QE_TRACE_SYS": "4"}, {"QE_TRACE_SYS": "0"},
              {"QE_FORMAT_WAVE": "1"}, {"QE_FORMAT_WAVE": "0"}]


@pytest.mark.parametrize("env", FILL_FORMS, ids=ident)
@pytest.mark.parametrize("name", FILL_SETS)
def test_fill_traceback_and_formatter_forms(name, env, monkeypatch):
    setenv(monkeypatch, env)
    scores, status, cig, cnt = gpu_batch(batch_of(pairs()), **U.PARAM_SETS[name])
    compare(name, status, scores, cig, ident(env))
    # the counters the forced tests of these switches compare (test_gpu_parity.py): the fill's block advances, and for
    # QuickEd the traceback's steps
    if not ({"QE_FILL_MULTI", "QE_FORMAT_WAVE"} & set(env)):
        assert cnt[1] == work_of(name, "fill_block_advances"), (name, env)
        if name == "quicked" and ({"QE_FILL_SYS", "QE_TRACE_SYS"} & set(env)):
            assert cnt[3] == work_of(name, "traceback_steps"), (name, env)


SPLIT = 1 << 15     # ebb x tlen x 16 bytes (bpm_hirschberg.c:63): 1 000 bases at bandwidth 40 are ~130 KB, 500 x 1 000 more


@functools.lru_cache(maxsize=None)
def split_expected(name):
    """the oracle's Hirschberg with the same threshold -> per pair (status, score, RLE CIGAR, splits)"""
    kw = U.PARAM_SETS[name]
    lib = O.oracle()
    out = []
    for p, t in pairs():
        ops = C.create_string_buffer(len(p) + len(t) + 1)
        n = C.c_int64()
        tr = O.QoTrace()
        st = lib.qo_hirschberg(p, len(p), t, len(t), max(len(p), len(t)) * kw["bandwidth"] // 100, SPLIT, ops, C.byref(n), C.byref(tr))
        buf = C.create_string_buffer(2 * n.value + 16)
        lib.qo_cigar_rle(ops, n.value, buf)
        out.append((st, int(lib.qo_cigar_score(ops, n.value)), buf.value.decode(), int(tr.hirschberg_splits)))
    return out


@pytest.mark.parametrize("G", ["1", "4", "16"])
@pytest.mark.parametrize("name", ["hirschberg_bw40", "hirschberg_bw100"])
def test_hirschberg_joins_halves_of_unequal_lengths(name, G, monkeypatch):
    """QE_SPLIT_BYTES small enough that the pairs of 1 000 and 2 500 bases really split, the half passes by G lanes per task:
    status, score and CIGAR bytes are those of the oracle's Hirschberg at the same threshold, inside the domain.  (Not the
    distance everywhere: the join reads score-only half passes, whose band cuts a large indel misleads -- 1 000 x 1 250 with
    its surplus in the middle joins to 352 at this threshold, the distance is 278; the reference's join is the same one.)"""
    _, exp, dom = expected(name)
    want = split_expected(name)
    big = [i for i, (p, t) in enumerate(pairs()) if len(p) >= 992]
    assert len(big) == 32 and all(want[i][3] > 0 for i in big)
    setenv(monkeypatch, {"QE_SPLIT_BYTES": str(SPLIT), "QE_COOP_G": G})
    scores, status, cig, _ = gpu_batch(batch_of(pairs()), **U.PARAM_SETS[name])
    n = 0
    for i, (p, t) in enumerate(pairs()):
        if not dom[i] or want[i][0] != O.OK:      # (a split that does not converge at this threshold: unspecified)
            continue
        assert (int(status[i]), int(scores[i]), cig[i]) == want[i][:3], (name, G, i + 1, len(p), len(t), want[i][3])
        n += 1
    assert n >= U.MIN_INSIDE[name] - 4 and sum(1 for i in big if dom[i] and want[i][0] == O.OK) >= 16, (name, n)
    # equal bytes show that the library did split: the oracle's CIGAR at its own threshold (no split below 16 MB) is another
    assert sum(1 for i in big if dom[i] and want[i][0] == O.OK and want[i][2] != exp[i][2]) >= 4


WINDOWED_FORMS = [{k: v} for k in ("QE_WINDOWED_CP", "QE_WINDOWED_QUAD", "QE_WINDOWED_SYS") for v in ("1", "0")]


@pytest.mark.parametrize("env", WINDOWED_FORMS, ids=ident)
@pytest.mark.parametrize("name", WINDOWED_SETS)
def test_windowed_forms(name, env, monkeypatch):
    setenv(monkeypatch, env)
    scores, status, cig, cnt = gpu_batch(batch_of(pairs()), **U.PARAM_SETS[name])
    compare(name, status, scores, cig, ident(env))
    assert cnt[2] == work_of(name, "window_block_steps"), (name, env)


def _three_runs(name, label, **more):
    """a resident batch's first run is host-driven, its second (waited for) and third (queued, then fetched) take the fast flow"""
    kw = dict(U.PARAM_SETS[name], **more)
    rb = capi.ResidentBatch(batch_of(pairs()))
    try:
        for rep in range(3):
            assert rb.run(capi.make_params(**kw), sync=rep < 2) >= 0
            if rep == 2:
                assert rb.fetch() >= 0
            scores, status = rb.scores()
            compare(name, status, scores, None if kw.get("only_score") else rb.cigars(), (label, rep), **more)
    finally:
        rb.close()


@pytest.mark.parametrize("env", [{k: v} for k in ("QE_QUICKED_FAST", "QE_STAGE3_DEVICE") for v in ("1", "0")], ids=ident)
@pytest.mark.parametrize("name", ["quicked", "quicked_scalar"])
def test_quicked_flows(name, env, monkeypatch):
    setenv(monkeypatch, env)
    _three_runs(name, ident(env))


@pytest.mark.parametrize("mode", ["1", "0"])
@pytest.mark.parametrize("name", ["quicked", "quicked_scalar"])
def test_quicked_score_pass(name, mode, monkeypatch):
    monkeypatch.setenv("QE_QUICKED_SCORE_PASS", mode)
    _three_runs(name, ("score pass", mode), only_score=True)
    al = capi.QuickedAligner()
    for k, v in dict(U.PARAM_SETS[name], only_score=True).items():
        setattr(al._params, k, v)
    st, out = al.alignBatch(list(pairs()))
    compare(name, [o[0] for o in out], [o[1] for o in out], None, ("score pass", mode, "alignBatch"), only_score=True)
    # which of the two ran, as test_quicked_only_score_pass tells: the pass walks no traceback
    _, _, _, cnt = gpu_batch(batch_of(pairs()), **dict(U.PARAM_SETS[name], only_score=True))
    assert (cnt[3] == 0) == (mode == "1"), (name, mode, [int(c) for c in cnt])


# ---------------------------------------------------------------------------------------------------------------------
# (c) per-pair statistics: with lengths this far apart, exchanging the roles of I and D cannot satisfy them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded_bw100", "quicked"])
def test_pair_statistics_identities(name):
    rb = capi.ResidentBatch(batch_of(pairs()))
    try:
        assert rb.configure(0) == 0 and rb.configure_tags(stats=True) == 0
        assert rb.run(capi.make_params(**U.PARAM_SETS[name]), sync=True) >= 0
        scores, status = rb.scores()
        cig = rb.cigars()
        compare(name, status, scores, cig, "statistics")
        stats = rb.pair_stats()
        for i, (p, t) in enumerate(pairs()):
            matches, mismatches, ins_bases, del_bases = (int(x) for x in stats[i][:4])
            m, n, score = len(p), len(t), int(scores[i])
            where = (name, i + 1, m, n, stats[i].tolist())
            assert matches + mismatches + del_bases == m, where
            assert matches + mismatches + ins_bases == n, where
            assert mismatches + ins_bases + del_bases == score, where
            assert ins_bases - del_bases == n - m, where
            assert tuple(int(x) for x in stats[i]) == T.expected_from_cigars([(p, t)], [cig[i]])[0][0], where
    finally:
        rb.close()
