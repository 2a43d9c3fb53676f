"""Panel search, a member cut off by the text's end (QUICKED_PANEL_TAILS): the definition, from the full matrix.

Text i has n >= 1 bases, member p has m bases and the effective bound k = min(bound, m).  D is the INFIX edit-distance matrix of
the member (rows) against the text (columns), D[0][j] = 0, under the run's equality.  Row r is a tail of p when

    min_overlap <= r <= m - 1   and   D[r][n] <= floor(r * k / m).

The member's tail is the tail row with the largest r - D[r][n], on a tie the smaller D[r][n]; the text's tail is the best
member's by the same two keys, then the smaller member index.  The record is (pattern, overlap r, text_start, score D[r][n]) with
text_start the smallest s for which the global distance of member[0:r] against text[s:n] is the score; (-1, -1, -1, -1) where no
member has a tail, and for an empty text.

The equalities: flag 0 folds case, A C G T equal themselves and any two other bytes are equal; under IUPAC the letters' base
sets intersect; under IUPAC_PATTERN the text's letters other than A C G T U are the empty set.  The symbol tables are
tests/iupac_lib.py's; every matrix is computed here, cell for cell.  It shares no code with quicked_amd/csrc.
"""
import numpy as np

import iupac_lib as I

INFIX = 2
IUPAC, IUPAC_PATTERN = I.IUPAC, I.IUPAC_PATTERN
TAILS = 2048
NONE = (-1, -1, -1, -1)
TAIL_FIELDS = ("pattern", "overlap", "text_start", "score")

_CODE = np.full(256, 4, dtype=np.int8)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k
    _CODE[_c + 32] = _k


def equal(pattern, text, flag):
    """-> (m, n) bool: member symbol i equals text symbol j under the run's equality"""
    if flag:
        return (I.masks(pattern, "p", flag)[:, None] & I.masks(text, "t", flag)[None, :]) != 0
    pc, tc = _CODE[np.frombuffer(bytes(pattern), dtype=np.uint8)], _CODE[np.frombuffer(bytes(text), dtype=np.uint8)]
    return pc[:, None] == tc[None, :]


def matrix(eq, prefix=False):
    """the full matrix D[0 .. m][0 .. n]: top row zeros (INFIX) or j (prefix), first column i"""
    m, n = eq.shape
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    idx = np.arange(n + 1, dtype=np.int64)
    if prefix:
        D[0] = idx
    for i in range(1, m + 1):
        tmp = np.empty(n + 1, dtype=np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (~eq[i - 1]).astype(np.int64))
        D[i] = np.minimum.accumulate(tmp - idx) + idx          # ... and D[i][j - 1] + 1, along the row
    return D


_COLS = {}


def last_column(pattern, text, flag):
    """D[0 .. m][n] of the INFIX matrix"""
    key = (bytes(pattern), bytes(text), flag)
    if key not in _COLS:
        _COLS[key] = matrix(equal(pattern, text, flag))[:, -1].copy()
    return _COLS[key]


def member_tail(col, m, bound, min_overlap):
    """column n of one member -> (overlap, score) of the member's tail, or None"""
    k = min(int(bound), m)
    rows = [(r, int(col[r])) for r in range(max(1, min_overlap), m) if int(col[r]) <= (r * k) // m]
    if not rows:
        return None
    return min(rows, key=lambda x: (-(x[0] - x[1]), x[1]))


def start_of(prefix, text, score, flag):
    """the smallest s for which the global distance of `prefix` against text[s:] is `score`"""
    n = len(text)
    back = matrix(equal(prefix[::-1], text[::-1], flag), prefix=True)[-1]      # back[j]: the distance to text[n - j:]
    js = np.nonzero(back == score)[0]
    assert len(js), (prefix, text, score)
    return n - int(js.max())


def text_tail(text, panel, bounds, flag, min_overlap):
    """-> (pattern, overlap, text_start, score) of one text, or NONE"""
    if not text:
        return NONE
    best = None
    for p, q in enumerate(panel):
        t = member_tail(last_column(q, text, flag), len(q), bounds[p], min_overlap)
        if t is not None:
            key = (-(t[0] - t[1]), t[1], p)
            if best is None or key < best[0]:
                best = (key, p, t[0], t[1])
    if best is None:
        return NONE
    _, p, r, d = best
    return (p, r, start_of(bytes(panel[p])[:r], bytes(text), d, flag), d)


def all_tails(texts, panel, bounds, flag, min_overlap):
    return [text_tail(t, panel, bounds, flag, min_overlap) for t in texts]


def cases_file(path, groups, flags, overlaps):
    """the input of the native programs (tests/native/panel_tails_cpu.cpp, panel_tails_host.cpp): the number of groups, and
    per group "K n nconf", K x {member bound}, n x text ("." = empty) and per (flag, min_overlap) "flag min_overlap" and n x
    {pattern overlap text_start score}, as this module defines them"""
    lines = ["%d" % len(groups)]
    for g in groups:
        texts, panel = g["texts"], g["panel"]
        lines.append("%d %d %d" % (len(panel), len(texts), len(flags) * len(overlaps)))
        lines += ["%s %d" % (q.decode(), b) for q, b in zip(panel, g["bounds"])]
        lines += [t.decode() or "." for t in texts]
        for flag in flags:
            for mo in overlaps:
                lines.append("%d %d" % (flag, mo))
                lines += [" ".join(str(int(v)) for v in t) for t in g["tails"][(flag, mo)]]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
