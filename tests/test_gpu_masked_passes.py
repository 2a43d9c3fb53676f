"""Masked multi-slot passes of k_banded<false> on the GPU (QE_SCORE_MASKED): BandEd score-only through the
C-ABI on the one-lane kernel, on bands whose heights differ inside every wave.  Scores are the oracle's, every status is
WIP, and counters[0] is the oracle's block-advance sum -- a dead slot is never counted -- under the all-or-none rule
(QE_SCORE_MASKED=0) and under the default, both alike.
tests/test_masked_passes_cpu.py walks the same inputs on the CPU and asserts that they contain passes with 0 < nl < K."""
import numpy as np
import pytest

import masked_lib as ML
import oracle_lib as O
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu


def batch_of(pairs):
    pp = np.frombuffer(b"".join(p for p, _ in pairs), dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs), dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1], dtype=np.int64)]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1], dtype=np.int64)]).astype(np.int64)
    return datagen.PairBatch(pp, po, pl, tp, to, tl)


def run(batch):
    rb = capi.ResidentBatch(batch)
    try:
        st = rb.run(capi.make_params(algo=2, only_score=True, bandwidth=ML.BW), sync=True)
        assert st >= 0, st
        scores, status = rb.scores()
        return scores.tolist(), status.copy(), rb.counters().copy()
    finally:
        rb.close()


def counters(cnt):
    return int(cnt[0]), int(cnt[7])


@pytest.mark.parametrize("name", list(ML.CASES))
def test_masked_passes_equal_the_oracle(monkeypatch, name):
    pairs, env, (exp_score, exp_adv, exp_miss), _ = ML.case(name)
    for k, v in {**ML.ONE_LANE, **env}.items():
        monkeypatch.setenv(k, v)
    batch = batch_of(pairs)
    seen = {}
    for masked in ("0", None):
        if masked is None:
            monkeypatch.delenv("QE_SCORE_MASKED", raising=False)
        else:
            monkeypatch.setenv("QE_SCORE_MASKED", masked)
        scores, status, cnt = run(batch)
        print(name, "QE_SCORE_MASKED", masked, "adv", counters(cnt)[0], "expected", exp_adv, "second-pass tasks", counters(cnt)[1])
        assert scores == exp_score, (name, masked)
        assert (status == O.WIP).all(), (name, masked)
        assert counters(cnt) == (exp_adv, exp_miss), (name, masked)
        seen[masked] = (scores, status.tolist(), counters(cnt))
    assert seen["0"] == seen[None]
