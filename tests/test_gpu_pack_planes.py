"""k_pack on the GPU, plane by plane (quicked_debug_pack -> capi.debug_pack): the planes, the two padding rows, the word
offsets and the flags of every sequence of tests/pack_lib.py -- every length across the boundaries of the scheme in six
alphabets, all 256 byte values at every position of a lane -- against the scalar rule in numpy, forward and reversed, through
the ONE launch that packs a batch's patterns and its texts; a pair's flags are the OR of its two sequences'.  Then a batch
of 300 pairs of 1.5 kb twice through ResidentBatch.run, so both parities of the plane sets see that launch: the oracle's
scores."""
import numpy as np
import pytest

import oracle_lib as O
import pack_lib as P
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets():
    """patterns = the sequences, texts = the same in another order: the two sequences of a pair have unequal counts of spans"""
    pats = P.sequences()
    order = np.random.default_rng(3).permutation(len(pats))
    texts = [pats[i] for i in order]
    ref = {rev: (P.ref_pack_set(pats, rev), P.ref_pack_set(texts, rev)) for rev in (False, True)}
    return pats, texts, ref


def _mismatch(got, exp, off, seqs):
    bad = np.nonzero(got != exp)[0]
    if len(bad) == 0:
        return None
    k = int(np.searchsorted(off, bad[0], side="right") - 1)
    return dict(sequence=k, length=len(seqs[k]), word=int(bad[0] - off[k]), got=hex(int(got[bad[0]])), exp=hex(int(exp[bad[0]])), mismatches=len(bad))


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_planes_padding_offsets_and_flags(sets, reverse):
    pats, texts, ref = sets
    (pw, poff, pfl), (tw, toff, tfl) = ref[reverse]
    gpw, gpoff, gtw, gtoff, gfl = capi.debug_pack(pats, texts, reverse=reverse)
    assert (gpoff == poff).all() and (gtoff == toff).all()
    assert len(gpw) == len(pw) and len(gtw) == len(tw)
    assert _mismatch(gpw, pw, poff, pats) is None, _mismatch(gpw, pw, poff, pats)
    assert _mismatch(gtw, tw, toff, texts) is None, _mismatch(gtw, tw, toff, texts)
    # the two rows behind every sequence are zeros
    for words, off, seqs in ((gpw, gpoff, pats), (gtw, gtoff, texts)):
        for k in (0, len(seqs) // 2, len(seqs) - 1):
            end = int(off[k]) + 3 * P.rows_of(len(seqs[k]))
            assert not words[end - 6:end].any()
    assert (gfl == (pfl | tfl)).all(), np.nonzero(gfl != (pfl | tfl))[0][:8]
    assert len(np.unique(pfl | tfl)) == 4                       # every combination of the two flags occurs


def test_a_pairs_flags_are_those_of_both_sequences():
    clean, lower, n_only, iupac = b"ACGT" * 300, b"ACGT" * 150 + b"acgt" * 150, b"ACGT" * 299 + b"NNNN", b"ACGT" * 299 + b"ACRT"
    pats = [clean, lower, clean, n_only, clean, iupac, lower, clean]
    texts = [clean, clean, lower, clean, n_only, clean, n_only, clean[:0]]
    assert [P.ref_pack(s)[1] for s in (clean, lower, n_only, iupac)] == [0, P.FLAG_NONCANON, P.FLAG_HAS_N, P.FLAG_HAS_N | P.FLAG_NONCANON]
    for reverse in (False, True):
        assert capi.debug_pack(pats, texts, reverse=reverse)[4].tolist() == [0, 2, 2, 1, 1, 3, 3, 0]


def test_both_parities_of_the_plane_sets_score_like_the_oracle():
    batch = datagen.generate(count=300, length=1500, error=0.05, seed=11)
    pairs = list(batch.pairs())
    exp = [O.oracle_align(p, t, algo=O.BANDED, only_score=True)[1] for p, t in pairs]
    rb = capi.ResidentBatch(batch)
    try:
        p = capi.make_params(algo=capi.BANDED, only_score=True)
        for _ in range(2):
            assert rb.run(p, sync=True) == capi.QUICKED_WIP
            scores, _status = rb.scores()
            assert scores.tolist() == exp
    finally:
        rb.close()
