"""Panel search, a member cut off by the text's start (QUICKED_PANEL_HEADS): the definition, in one sentence.

The heads of (texts, panel) are the tails of (reversed texts, reversed members) as tests/panel_tails_lib.py defines them -- the
full INFIX matrix of rev(member) against rev(text), row r a head when min_overlap <= r <= m - 1 and D^R[r][n] <= floor(r k / m),
the largest matched length r - D^R[r][n], then the smaller score, then the smaller member index -- with text_end = n - text_start:
the member's last r bases fit text[0:text_end), the longest such stretch.  rev() is plain reversal, no complement.  The record is
(pattern, overlap r, text_end, score); (-1, -1, -1, -1) where no member has a head, and for an empty text.

Nothing here comes from quicked_amd/csrc; every matrix is panel_tails_lib's, cell for cell.
"""
import panel_tails_lib as T

INFIX, PREFIX = 2, 1
IUPAC, IUPAC_PATTERN = T.IUPAC, T.IUPAC_PATTERN
HEADS = 8192
NONE = T.NONE
HEAD_FIELDS = ("pattern", "overlap", "text_end", "score")


def text_head(text, panel, bounds, flag, min_overlap):
    """-> (pattern, overlap, text_end, score) of one text, or NONE"""
    text = bytes(text)
    t = T.text_tail(text[::-1], [bytes(q)[::-1] for q in panel], bounds, flag, min_overlap)
    if t == T.NONE:
        return NONE
    p, r, s, d = t
    return (p, r, len(text) - s, d)


def all_heads(texts, panel, bounds, flag, min_overlap):
    return [text_head(t, panel, bounds, flag, min_overlap) for t in texts]


def reach(member, bound):
    """the text columns a head of this member can depend on: m + k, k = min(bound, m)"""
    return len(member) + min(int(bound), len(member))


def cases_file(path, groups, flags, overlaps):
    """the input of the native programs (tests/native/panel_heads_cpu.cpp, panel_heads_host.cpp): panel_tails_lib.cases_file's
    layout with the heads {pattern overlap text_end score} in the tails' place"""
    T.cases_file(path, [dict(g, tails=g["heads"]) for g in groups], flags, overlaps)
