"""Every occurrence within the bound (quicked_batch_run_search_all): the definition as a plain loop, and edlib's HW / SHW
location lists.

The loop is include/quicked_batch.h's text: R[e] = D[m][e] from search_lib.last_row (the brute-force DP), k = min(bound, m);
position e is an occurrence when R[e] <= k, R[e] < R[e - 1] (column 0 counts as higher than every value) and the first later
column with another value, if there is one, has a higher one.  text_start is 0 for PREFIX; for INFIX the smallest s for which
the global distance of the pattern against text[s:e] is the occurrence's score, computed on the stretch of the last
min(e, m + score) columns -- no stretch is longer.  It shares no code with quicked_amd/csrc/qe_search.h.
"""
import ctypes as C

import numpy as np

import search_lib as S

PREFIX, INFIX = S.PREFIX, S.INFIX


def valleys(row, k):
    """row = R[1 .. n] -> [(e, R[e])] of the definition"""
    n = len(row)
    out = []
    for e in range(1, n + 1):
        v = int(row[e - 1])
        if v > k:
            continue
        if e > 1 and not v < int(row[e - 2]):
            continue
        j = e                                     # row[j] is column j + 1
        while j < n and int(row[j]) == v:
            j += 1
        if j < n and int(row[j]) < v:
            continue
        out.append((e, v))
    return out


def start_of(pattern, text, e, score):
    m = len(pattern)
    w = min(e, m + score)
    back = S.last_row(pattern[::-1], text[e - w:e][::-1], True)[1:]       # back[j - 1]: the global distance to text[e - j:e]
    assert int(back.min()) == score, (m, e, score, int(back.min()))
    return e - (int(np.nonzero(back == score)[0][-1]) + 1)


_ROWS = {}


def row_of(pattern, text, mode):
    key = (pattern, text, mode)
    if key not in _ROWS:
        _ROWS[key] = S.last_row(pattern, text, mode == PREFIX)[1:]
    return _ROWS[key]


_STARTS = {}


def occurrences(pattern, text, mode, bound):
    """-> [(text_start, text_end, score)] ordered by text_end"""
    k = min(int(bound), len(pattern))
    out = []
    for e, v in valleys(row_of(pattern, text, mode), k):
        if mode == PREFIX:
            out.append((0, e, v))
            continue
        key = (pattern, text, e, v)
        if key not in _STARTS:
            _STARTS[key] = start_of(pattern, text, e, v)
        out.append((_STARTS[key], e, v))
    return out


def best_of(occ):
    """the smallest score among the occurrences and the first occurrence that has it: (score, start, end), or (-1, -1, -1)"""
    if not occ:
        return (-1, -1, -1)
    d = min(o[2] for o in occ)
    s, e, _ = next(o for o in occ if o[2] == d)
    return (d, s, e)


def filter_runs(ends):
    """a sorted list of end positions with every member whose predecessor is also in the list removed"""
    have = set(ends)
    return [e for e in ends if e - 1 not in have]


# ---- edlib: every location of the best distance ----------------------------------------------------------------------
def edlib_all(pattern, text, mode):
    """-> (d, [(startLocations[i], endLocations[i] + 1)]) with EDLIB_TASK_LOC and no bound"""
    if S._edlib is None:
        S.edlib_locate(b"A", b"A", INFIX)         # loads the library and sets the prototypes
    r = S._edlib.edlibAlign(bytes(pattern), len(pattern), bytes(text), len(text),
                            S.EdlibAlignConfig(-1, S.EDLIB_MODE[mode], S.EDLIB_TASK_LOC, None, 0))
    assert r.status == 0
    out = [(int(r.startLocations[i]), int(r.endLocations[i]) + 1) for i in range(r.numLocations)]
    d = int(r.editDistance)
    S._edlib.edlibFreeAlignResult(r)
    return d, out


def edlib_best_occurrences(pattern, text, mode):
    """edlib's view of the occurrences of the best score: its end list with runs of neighbouring ends reduced to their
    first member, and its starts of those ends -> (d, [[start, end]]); None where edlib cannot judge (d == m)"""
    d, locs = edlib_all(pattern, text, mode)
    if d == len(pattern):
        return None
    ends = sorted({e for _, e in locs})
    keep = set(filter_runs(ends))
    return d, [[s, e] for s, e in locs if e in keep]
