"""The CIGAR validator on the GPU: what k_check_strings (quicked_batch_validate) and k_check_segs (the in-run check) REJECT.
Expected verdicts never come from the library: they are the rules restated in tests/check_lib.py, which the CPU suite pins
to the oracle's cigar_check_alignment; the cases are check_lib's too, and tests/test_check_cpu.py has run every one of them
through the same source (quicked_amd/csrc/qe_check.h) under the sanitizers.  Strings whose run lengths could take a walk
that adds in 32 bits outside its pair are not here: they stay on the CPU.

Shapes are small: pairs of 0 to 300 bases, fewer than 2 000 per batch.  One pair is larger: "1M1I1D" repeated to 200 000
characters consumes 66 666 bases of each sequence, so the string the plumbing test asks for on a 300-base pair is there with
zero-padded lengths, and in its plain form on the pair it needs."""
import numpy as np
import pytest

import check_lib as L
from quicked_amd import capi, datagen

pytestmark = pytest.mark.gpu


def _batch(pairs):
    """the pairs back to back, no padding: a pair starts wherever the one before it ended"""
    pp = np.frombuffer(b"".join(p for p, _ in pairs) or b"\0", dtype=np.uint8).copy()
    tp = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8).copy()
    pl = np.array([len(p) for p, _ in pairs], dtype=np.int32)
    tl = np.array([len(t) for _, t in pairs], dtype=np.int32)
    po = np.concatenate([[0], np.cumsum(pl[:-1])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tl[:-1])]).astype(np.int64)
    return datagen.PairBatch(pp, po, pl, tp, to, tl)


def _validate(rb, strings, terminate_last=True, fill=0, break_offset=None):
    """quicked_batch_validate itself -> (status, verdicts); the pool is built here so that a test can leave the last
    terminator out or point an offset past the pool"""
    off = np.full(rb.n, -1, dtype=np.int64)
    blob = bytearray()
    for i, s in enumerate(strings):
        if s is not None:
            off[i] = len(blob)
            blob += s.encode("latin-1") + b"\0"
    if not terminate_last:
        blob = blob[:-1]
    if break_offset is not None:
        off[break_offset[0]] = len(blob) + break_offset[1]
    ok = np.full(rb.n, fill, dtype=np.int32)
    st = rb._lib.quicked_batch_validate(rb._h, bytes(blob), len(blob), off.ctypes.data, ok.ctypes.data)
    return st, ok


def _judge(cases):
    """one batch of the cases' pairs, one validate call over their strings -> verdicts"""
    assert 0 < len(cases) < 2000
    rb = capi.ResidentBatch(_batch([(p, t) for _, p, t, _ in cases]))
    st, got = _validate(rb, [s for _, _, _, s in cases])
    rb.close()
    assert st == capi.QUICKED_OK
    return [int(x) for x in got]


def _want(cases):
    return [L.verdict(p, t, s) for _, p, t, s in cases]


def _assert_verdicts(cases, got, want=None):
    want = _want(cases) if want is None else want
    bad = [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])


SHIFT = ("one byte in front", b"A", b"C", "1X")      # moves every pair behind it to the other parity of pool offsets


def test_every_byte_lane_of_the_m_compare():
    cases = L.byte_lane_cases()
    for shift in (0, 1):
        batch = [SHIFT] * shift + cases
        got = _judge(batch)
        _assert_verdicts(batch, got)
        for c, g in zip(batch[shift:], got[shift:]):
            assert g == (0 if c[0].endswith(" M") else 1), c[0]
    # the pairs of one length lie back to back, so with and without the byte in front every length >= 8 has had its
    # 8-byte loads at odd and at even addresses
    assert len(cases) == 2 * (1 + 7 + 8 + 9 + 16 + 17 + 23)


def test_x_branch():
    cases = L.x_branch_cases()
    got = _judge(cases)
    _assert_verdicts(cases, got)
    for c, g in zip(cases, got):
        assert g == (1 if c[0].endswith("all different") else 0), c[0]
    assert {c[0].split()[1] for c in cases} == {"len=1", "len=2", "len=9"}


def test_counts_one_off_and_misplaced_runs():
    good, mutants = L.count_cases()
    cases = good + mutants
    want = _want(cases)
    assert all(w == 1 for w in want[:len(good)])
    invalid = want[len(good):].count(0)
    assert invalid >= 0.95 * len(mutants) and len(mutants) > 300, (invalid, len(mutants))      # the mutators still mutate
    _assert_verdicts(cases, _judge(cases), want)


def test_raw_bytes():
    cases = L.raw_byte_cases()
    want = _want(cases)
    by_label = {c[0]: w for c, w in zip(cases, want)}
    assert (by_label["a vs A as M"], by_label["a vs A as X"], by_label["N vs N as M"], by_label["N vs N as X"]) == (0, 1, 1, 0)
    assert any(b in c[1] for c in cases for b in (0x00, 0x80, 0xFF))
    _assert_verdicts(cases, _judge(cases), want)


def test_syntax_and_the_length_limit():
    cases = L.syntax_cases() + L.length_cases(False)
    want = _want(cases)
    by_string = {c[3]: w for c, w in zip(cases, want) if c[0].startswith("syntax")}
    assert by_string["7M"] == 1 and by_string["007M"] == 1 and by_string["7="] == 1
    for s in ("7", "M", "0M", "7Q", "7m", " 7M", "-1M", "2147483648M", "123456789012345678901234567890M"):
        assert by_string[s] == 0, s
    assert want[:2] == [1, 0]                                   # "" on an empty and on a non-empty pair
    _assert_verdicts(cases, _judge(cases), want)


def test_run_lengths_whose_sums_wrap_back_into_range():
    """I and D runs of 2^31 - 1 that a 32-bit sum brings back to the start before any base is compared: verdict 0"""
    cases = L.wrap_cases_in_range()
    assert len(cases) >= 36 and set(_want(cases)) == {0}
    _assert_verdicts(cases, _judge(cases))


def test_plumbing():
    p7 = b"ACGTACG"
    pairs = [(p7, p7)] * 5
    rb = capi.ResidentBatch(_batch(pairs))
    # no string: -1, whatever its neighbours are
    st, got = _validate(rb, ["7M", None, "6M", None, "7M"], fill=7)
    assert st == capi.QUICKED_OK and got.tolist() == [1, -1, 0, -1, 1]
    st, got = _validate(rb, [None] * 5, fill=7)
    assert st == capi.QUICKED_OK and got.tolist() == [-1] * 5
    # an offset at or past the end of the pool: an error, and nothing is written
    for past in (0, 1, 1 << 40):
        st, got = _validate(rb, ["7M"] * 5, fill=7, break_offset=(2, past))
        assert st == capi.QUICKED_ERROR and got.tolist() == [7] * 5, past
    # the last string of the pool without its terminator is judged on its content
    st, got = _validate(rb, ["7M", "7M", "7M", "7M", "3M4M"], terminate_last=False)
    assert st == capi.QUICKED_OK and got.tolist() == [1] * 5
    st, got = _validate(rb, ["7M", "7M", "7M", "7M", "3M4"], terminate_last=False)
    assert st == capi.QUICKED_OK and got.tolist() == [1, 1, 1, 1, 0]
    st, got = _validate(rb, ["7M", "7M", None, None, "7M1"], terminate_last=False)
    assert st == capi.QUICKED_OK and got.tolist() == [1, 1, -1, -1, 0]
    rb.close()
    # one lane with 200 000 characters to read, its neighbours with two
    longs = L.long_string_cases()
    assert all(len(c[3]) == 200000 for c in longs) and (len(longs[0][1]), len(longs[0][2])) == (300, 300)
    cases = [("short", p7, p7, "7M"), longs[0], ("short", p7, p7, "6M"), longs[1], longs[2], ("short", p7, p7, "7M"), longs[3]]
    want = _want(cases)
    assert want == [1, 1, 0, 0, 1, 1, 0]
    _assert_verdicts(cases, _judge(cases), want)


def test_a_lanes_verdict_does_not_depend_on_its_neighbours():
    """everything above in one batch, in a seeded shuffled order and then reversed: every verdict is its stand-alone one"""
    cases = L.gpu_cases() + [(f"no string {k}", b"ACGT", b"ACGT", None) for k in range(40)]
    assert 64 < len(cases) < 2000 and len(cases) % 64 != 0
    order = np.random.default_rng(5301).permutation(len(cases)).tolist()
    want = _want(cases)
    assert want.count(1) > 100 and want.count(0) > 300 and want.count(-1) == 40
    for idx in (order, order[::-1]):
        batch = [cases[k] for k in idx]
        _assert_verdicts(batch, _judge(batch), [want[k] for k in idx])


# ---- the in-run form against the string form -----------------------------------------------------------------------------
ALGOS = {"quicked": dict(algo=capi.QUICKED), "banded": dict(algo=capi.BANDED), "windowed_w2": dict(algo=capi.WINDOWED, window_size=2),
         "hirschberg": dict(algo=capi.HIRSCHBERG)}
_memo = {}


def run_pairs():
    """150 pairs of 300 to 1 200 bases: 120 at 8-10 % error, and 30 whose optimal alignment has no mismatch (equal; one base
    inserted; one base deleted), so that the style-2 strings of both kinds are there"""
    if "pairs" not in _memo:
        rng = np.random.default_rng(5302)
        pairs = []
        for k in range(150):
            p = L.random_seq(rng, int(rng.integers(300, 1201)))
            if k % 5 != 0:
                t = L.mutate_with_runs(rng, p, 0.08 + 0.02 * rng.random())[0]
            elif k % 15 == 0:
                t = p
            else:
                j = int(rng.integers(1, len(p) - 1))
                t = p[:j] + p[j + 1:] if k % 15 == 5 else p[:j] + bytes([int(rng.choice(list(b"ACGT")))]) + p[j:]
            pairs.append((p, t))
        _memo["pairs"] = pairs
    return _memo["pairs"]


@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_in_run_and_string_forms_agree(algo, monkeypatch):
    if algo == "hirschberg":
        monkeypatch.setenv("QE_SPLIT_BYTES", "4096")            # roots made of several segments
    pairs = run_pairs()
    assert len(pairs) == 150 and all(300 <= len(p) <= 1200 for p, _ in pairs)
    rb = capi.ResidentBatch(_batch(pairs))
    params = capi.make_params(**ALGOS[algo])
    by_style = {}
    for style in (0, 1, 2):
        assert rb.configure(cigar_style=style, check=True) == 0
        assert rb.run(params, sync=True) >= 0
        by_style[style] = (rb.cigars(), rb.check_results().tolist())
        by_style[style] += (rb.validate(by_style[style][0]).tolist(),)
    rb.close()
    have = [c is not None for c in by_style[0][0]]
    assert sum(have) >= 140, sum(have)
    for style in (0, 1):
        cg, in_run, from_string = by_style[style]
        for i, (p, t) in enumerate(pairs):
            assert (cg[i] is not None) == have[i]
            want = L.verdict(p, t, cg[i])
            assert in_run[i] == from_string[i] == want == (1 if have[i] else -1), (algo, style, i, in_run[i], from_string[i], want)
    # "MID": the alignment is as valid as before, the printed string -- X folded into M -- no longer says which bases differ
    cg, in_run, from_string = by_style[2]
    groups = {0: 0, 1: 0}
    for i, (p, t) in enumerate(pairs):
        if not have[i]:
            assert cg[i] is None and in_run[i] == from_string[i] == -1
            continue
        want = L.verdict(p, t, cg[i])
        has_x = "X" in by_style[0][0][i]
        assert in_run[i] == 1 and from_string[i] == want == (0 if has_x else 1), (algo, i, in_run[i], from_string[i], want, has_x)
        groups[want] += 1
    assert groups[0] > 0 and groups[1] > 0, groups
