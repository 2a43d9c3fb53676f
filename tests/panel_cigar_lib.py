"""The alignment of a stored occurrence (QUICKED_PANEL_CIGARS on quicked_batch_run_panel_all / _scan): the definition.

D is the full edit-distance matrix of the member (rows 1 .. m) against text[text_start:text_end] (columns 1 .. L) with
D[0][j] = j and D[i][0] = i, under the run's equality: unflagged, search_lib's codes (case folded, every byte that is not ACGT
one symbol); under a flag, iupac_lib's sets intersect.  From (m, L), while i > 0 and j > 0:
  1. D[i][j] == D[i-1][j] + 1     -> D, i -= 1
  2. D[i][j-1] == D[i-1][j-1] - 1 -> I, j -= 1
  3. else M where the two symbols are equal, X where not, both -= 1
then the columns left as I, the rows left as D; the operations are that sequence reversed.  Style 0 is their run-length string
over "MXID"; styles 1 and 2 are oracle_lib.sam_cigar of it.  It shares no code with quicked_amd/csrc/qe_panel_align.h.
"""
import re

import numpy as np

import iupac_lib as I
import oracle_lib as O
import search_lib as S

CIGARS = 512


def equal_matrix(member, stretch, flag):
    """[m][L] bool: row symbol i equal to column symbol j under the run's equality"""
    if flag:
        return (I.masks(member, "p", flag)[:, None] & I.masks(stretch, "t", flag)[None, :]) != 0
    return S.codes(member)[:, None] == S.codes(stretch)[None, :]


def matrix(eq):
    m, n = eq.shape
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    idx = np.arange(m + 1, dtype=np.int64)
    for j in range(1, n + 1):
        new = np.empty(m + 1, dtype=np.int64)
        new[0] = j
        np.minimum(D[1:, j - 1] + 1, D[:-1, j - 1] + (~eq[:, j - 1]), out=new[1:])
        D[:, j] = np.minimum.accumulate(new - idx) + idx
    return D


def operations(member, stretch, flag):
    """-> (score, the operations front to back as a str over "MXID")"""
    eq = equal_matrix(bytes(member), bytes(stretch), flag)
    D = matrix(eq)
    i, j = eq.shape
    out = []
    while i > 0 and j > 0:
        if D[i][j] == D[i - 1][j] + 1:
            out.append("D")
            i -= 1
        elif D[i][j - 1] == D[i - 1][j - 1] - 1:
            out.append("I")
            j -= 1
        else:
            out.append("M" if eq[i - 1][j - 1] else "X")
            i -= 1
            j -= 1
    out += ["I"] * j + ["D"] * i
    return int(D[-1][-1]), "".join(reversed(out))


def rle(ops):
    return "".join("%d%s" % (len(r.group(0)), r.group(1)) for r in re.finditer(r"(.)\1*", ops))


def styled(rle0, style):
    """the style-0 string in the batch's style (0, 1, 2)"""
    return rle0 if style == 0 else O.sam_cigar(rle0, style == 1)


def cigar(member, stretch, flag):
    """-> (score, the style-0 string)"""
    d, ops = operations(member, stretch, flag)
    return d, rle(ops)


def hit_cigars(text, panel, hits, flag):
    """one text's occurrences [(pattern, text_start, text_end, score)] -> their style-0 strings; asserts the scores"""
    out = []
    for p, s, e, v in hits:
        d, c = cigar(panel[p], text[s:e], flag)
        assert d == v, (p, s, e, v, d)
        out.append(c)
    return out


def invariants(c, style, m, length, score, prefix=False):
    """what every string must satisfy whatever the rule: edits, the consumed lengths, no trailing I and -- INFIX, where the stretch
    starts where the occurrence does; a PREFIX stretch starts at column 0 and its top row is counted -- no leading I"""
    runs = [(int(n), o) for n, o in re.findall(r"(\d+)([MXID=])", c)]
    assert "".join("%d%s" % r for r in runs) == c and runs, c
    assert sum(n for n, o in runs if o in "MX=D") == m and sum(n for n, o in runs if o in "MX=I") == length, (c, m, length)
    assert (prefix or runs[0][1] != "I") and runs[-1][1] != "I", c
    if style != 2:
        assert sum(n for n, o in runs if o in "XID") == score, (c, score)
    else:
        assert sum(n for n, o in runs if o in "ID") <= score, (c, score)


def cases_file(path, s, modes, flags, confs=("own", "uniform")):
    """the input of the native programs (tests/native/panel_cigar_cpu.cpp, panel_cigar_host.cpp): K n nconf, K x {member bound},
    n x text ("." = empty) and per (mode, flag, conf) "mode flag uniform" (-1: the members' own bounds) and n x {stored, stored x
    {pattern text_start text_end score, the string in styles 0, 1 and 2}}, uncapped"""
    texts, panel = s["texts"], s["panel"]
    lines = ["%d %d %d" % (len(panel), len(texts), len(modes) * len(flags) * len(confs))]
    lines += ["%s %d" % (q.decode(), b) for q, b in zip(panel, s["bounds"])]
    lines += [t.decode() or "." for t in texts]
    for mode in modes:
        for flag in flags:
            for conf in confs:
                lines.append("%d %d %d" % (mode, flag, -1 if conf == "own" else s["uniform"]))
                for hits, cigs in zip(s["hits"][(mode, flag, conf)], s["cigars"][(mode, flag, conf)]):
                    row = [str(len(hits))]
                    for o, c in zip(hits, cigs):
                        row += [str(int(v)) for v in o] + [styled(c, st) for st in (0, 1, 2)]
                    lines.append(" ".join(row))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
