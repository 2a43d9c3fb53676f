"""Eq from a table for the tall passes of the first launch (QE_SCORE_PEQ): k_banded<false, false, true> keeps a
per-lane Eq table of the pass's slots in LDS and the band state in the group workspace.  The twelve cases of
tests/test_gpu_score_tall.py (one template height each 5 .. 10, the ragged wave lane-relative and union, the general passes,
the ring-wrap set, the 13-slot edge, one pair alone), each with and without a forced prune, run the one-lane kernel under
QE_SCORE_NARROW=1 and a forced QE_NARROW_FIT once with QE_SCORE_PEQ=1 and once with 0: scores, statuses and
counters[0] / [7] are identical between the two and equal to the model of tests/narrow_prune_lib.py.  Which form ran is read
from the library's QE_TRACE line.  QE_SCORE_LDS stays unset: forced to 1 it asks for the form without the table."""
import re

import pytest

import masked_lib as ML
import narrow_fit_lib as FL
import oracle_lib as O
import test_gpu_score_tall as T

pytestmark = pytest.mark.gpu

work = T.work       # the walk of the model, compiled once per module; the cases' models are shared with test_gpu_score_tall.py

LINE = r"first launch of (\d+) groups, band state in (LDS|the group workspace) \((\d+) slots\), tall passes (on|off)(, Eq from a table in LDS)?"


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("name", list(T.CASES))
def test_table_form_equals_the_launch_without_it_and_the_oracle(monkeypatch, capfd, work, name, prune):
    pairs, env, k, kp, model = T.case(name, prune, work)
    exp = FL.totals(model)
    monkeypatch.delenv("QE_SCORE_LDS", raising=False)
    monkeypatch.delenv("QE_SCORE_TALL", raising=False)
    for key, v in dict(ML.ONE_LANE, QE_SCORE_NARROW="1", QE_NARROW_FIT=str(k), QE_NARROW_PRUNE=str(kp), QE_TRACE="1", **env).items():
        monkeypatch.setenv(key, v)
    batch = T.batch_of(pairs)
    groups = str((len(pairs) + 63) // 64)
    seen = {}
    for peq in ("1", "0"):
        monkeypatch.setenv("QE_SCORE_PEQ", peq)
        capfd.readouterr()
        scores, status, cnt = T.run(batch)
        err = capfd.readouterr().err
        form = re.findall(LINE, err)
        with capfd.disabled():
            print(name, "prune", kp, "QE_SCORE_PEQ", peq, form, "adv / second-pass tasks", cnt, "expected", exp[1:])
        # these lists are far below a group per SIMD: without the table the launch is the workspace form, no tall passes
        want = (groups, "the group workspace", "0", "on", ", Eq from a table in LDS") if peq == "1" else (groups, "the group workspace", "0", "off", "")
        assert form == [want], err[-2000:]
        assert scores == exp[0], (name, peq)
        assert status == [O.WIP] * len(pairs), (name, peq)
        assert cnt == (exp[1], exp[2]), (name, peq)
        seen[peq] = (scores, status, cnt)
    assert seen["1"] == seen["0"]
