"""Panel search (quicked_batch_run_panel): the definition, from the per-pair brute forces.

Per (text, member): search_lib's DP (the library's equality) or iupac_lib's (the two flags) gives the unbounded {d, text_end};
search_lib.bounded's rule cuts it at the member's bound (clamped to m).  Per text the members within their bound are ordered by
the key (score, panel index): the smallest is the best, the smallest of the others the runner-up, -1 where there is none.
text_start is the best member's: 0 for PREFIX, for INFIX the smallest s whose stretch text[s:text_end] has global distance
score.  An empty text has -1 everywhere.  It shares no code with quicked_amd/csrc/qe_panel.h or qe_search.h.
"""
import numpy as np

import iupac_lib as I
import search_lib as S

PREFIX, INFIX = S.PREFIX, S.INFIX
IUPAC, IUPAC_PATTERN = I.IUPAC, I.IUPAC_PATTERN
MATRIX = 64
INT32_MAX = 2**31 - 1
HIT_FIELDS = ("pattern", "score", "text_start", "text_end", "second_pattern", "second_score")


def pair_answer(pattern, text, mode, flag):
    """-> (d, text_end) of one member against one text, without a bound; flag 0 / IUPAC / IUPAC_PATTERN"""
    if flag:
        row = I.row_of(bytes(pattern), bytes(text), mode, flag)
    else:
        row = S.last_row(pattern, text, mode == PREFIX)[1:]
    d = int(row.min())
    return d, int(np.argmax(row == d)) + 1


def text_answers(text, panel, mode, flag):
    """pair_answer for every member at once -> (d [K], text_end [K]): the same DP with the members as the rows of one padded
    array (a padding row equals nothing, and no cell depends on a row below it), so that a test can afford thousands of pairs.
    tests/test_search_panel_cpu.py holds it to pair_answer."""
    k, width = len(panel), max(len(q) for q in panel)
    lens = np.array([len(q) for q in panel])
    if flag:
        rows = np.zeros((k, width), dtype=np.uint8)               # the empty set
        for p, q in enumerate(panel):
            rows[p, :len(q)] = I.masks(q, "p", flag)
        cols = I.masks(text, "t", flag)
    else:
        rows = np.full((k, width), 9, dtype=np.int8)               # no symbol
        for p, q in enumerate(panel):
            rows[p, :len(q)] = S.codes(q)
        cols = S.codes(text)
    idx = np.arange(width + 1, dtype=np.int64)
    col = np.tile(idx, (k, 1))
    new = np.empty_like(col)
    member = np.arange(k)
    best = np.full(k, np.iinfo(np.int64).max)
    end = np.zeros(k, dtype=np.int64)
    for j in range(1, len(text) + 1):
        differ = ((rows & cols[j - 1]) == 0) if flag else (rows != cols[j - 1])
        new[:, 0] = j if mode == PREFIX else 0
        np.minimum(col[:, 1:] + 1, col[:, :-1] + differ, out=new[:, 1:])
        col = np.minimum.accumulate(new - idx, axis=1) + idx
        v = col[member, lens]
        better = v < best
        best[better] = v[better]
        end[better] = j
    return best, end


def matrix(texts, panel, mode, flag):
    """-> (D, E) int64 [len(texts), len(panel)]: every pair's unbounded {d, text_end}; the row of an empty text is -1"""
    D = np.full((len(texts), len(panel)), -1, dtype=np.int64)
    E = np.full((len(texts), len(panel)), -1, dtype=np.int64)
    for i, t in enumerate(texts):
        if t:
            D[i], E[i] = text_answers(t, panel, mode, flag)
    return D, E


def cut(D, E, panel, bounds):
    """the matrix a run with these bounds (one per member) reports: {-1, -1} where d exceeds min(bound, m)"""
    D, E = np.array(D, dtype=np.int64), np.array(E, dtype=np.int64)
    for p, q in enumerate(panel):
        beyond = D[:, p] > min(int(bounds[p]), len(q))
        D[beyond, p] = -1
        E[beyond, p] = -1
    return D, E


def text_start(pattern, text, mode, flag, end, score):
    if mode == PREFIX:
        return 0
    if flag:
        return I.start_of(bytes(pattern), bytes(text), end, score, flag)
    w = min(end, len(pattern) + score)
    back = S.last_row(pattern[::-1], text[end - w:end][::-1], True)[1:]
    assert int(back.min()) == score
    return end - (int(np.nonzero(back == score)[0][-1]) + 1)


def reduce_text(drow, erow):
    """one text's bounded row -> (pattern, score, text_end, second_pattern, second_score) by the key order"""
    keys = sorted((int(d), p) for p, d in enumerate(drow) if d >= 0)
    if not keys:
        return -1, -1, -1, -1, -1
    best = keys[0]
    second = keys[1] if len(keys) > 1 else (-1, -1)
    return best[1], best[0], int(erow[best[1]]), second[1], second[0]


def expected(texts, panel, bounds, mode, flag, D=None, E=None):
    """-> (hits [n][6] in the order of HIT_FIELDS, Db, Eb): what a panel run reports; D / E: the unbounded matrix, if at hand"""
    if D is None:
        D, E = matrix(texts, panel, mode, flag)
    Db, Eb = cut(D, E, panel, bounds)
    hits = np.full((len(texts), 6), -1, dtype=np.int64)
    for i, t in enumerate(texts):
        if not t:
            continue
        p, s, e, p2, s2 = reduce_text(Db[i], Eb[i])
        if p < 0:
            continue
        hits[i] = (p, s, text_start(panel[p], t, mode, flag, e, s), e, p2, s2)
    return hits, Db, Eb


def cases_file(path, s, modes, flags):
    """the input of the native programs (tests/native/search_panel_cpu.cpp, search_panel_host.cpp): the set -- K n nconf, K x
    {member bound}, n x text ("." = empty) -- and per (mode, flag, the members' own bounds / the uniform one) "mode flag
    uniform" (-1: the own bounds) and n x {the 6 hit fields, K scores, K ends} as this module defines them"""
    texts, panel = s["texts"], s["panel"]
    lines = ["%d %d %d" % (len(panel), len(texts), len(modes) * len(flags) * 2)]
    lines += ["%s %d" % (q.decode(), b) for q, b in zip(panel, s["bounds"])]
    lines += [t.decode() or "." for t in texts]
    for mode in modes:
        for flag in flags:
            for uniform in (-1, s["uniform"]):
                bounds = s["bounds"] if uniform < 0 else [uniform] * len(panel)
                hits, Db, Eb = expected(texts, panel, bounds, mode, flag, *s["matrix"][(mode, flag)])
                lines.append("%d %d %d" % (mode, flag, uniform))
                for i in range(len(texts)):
                    lines.append(" ".join(str(int(v)) for v in list(hits[i]) + list(Db[i]) + list(Eb[i])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
