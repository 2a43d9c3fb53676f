"""IUPAC degenerate-base search (QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN): the definition as a brute-force DP, and
edlib with additionalEqualities.

The DP is include/quicked_batch.h's text: every byte stands for a set of bases (case folded; any byte outside the alphabet
the empty set), two symbols are equal when their sets intersect, and everything else -- the two modes, d, text_end the
smallest end, text_start the longest stretch, the occurrences as the valleys of row m -- is the unflagged search's.  The
flag decides the TEXT's table: IUPAC reads it like the pattern, IUPAC_PATTERN gives every text byte that is not one of
ACGTU the empty set.  It shares no code with quicked_amd/csrc/qe_iupac.h or qe_search.h.  edlib (oracle/_ref, where built),
with its additionalEqualities set to the 80 unordered pairs of distinct letters whose sets intersect, is the independent
opinion for IUPAC on upper-case input over the 15 letters, and for IUPAC_PATTERN where the text is upper-case ACGT.
"""
import ctypes as C

import numpy as np

import search_hits_lib as H
import search_lib as S

PREFIX, INFIX = S.PREFIX, S.INFIX
IUPAC, IUPAC_PATTERN = 16, 32
LETTERS = "ACGTRYSWKMBDHVN"
SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
        "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}

MASK = np.zeros(256, dtype=np.uint8)                 # the pattern's table, and the text's under IUPAC
for _l, _s in SETS.items():
    _v = sum(1 << "ACGT".index(b) for b in _s)
    MASK[ord(_l)] = _v
    MASK[ord(_l.lower())] = _v
MASK_ACGT = np.zeros(256, dtype=np.uint8)            # the text's under IUPAC_PATTERN
for _l in "ACGTUacgtu":
    MASK_ACGT[ord(_l)] = MASK[ord(_l)]


def masks(seq, side, flag):
    """side 'p' / 't'; flag IUPAC / IUPAC_PATTERN"""
    table = MASK_ACGT if (side == "t" and flag == IUPAC_PATTERN) else MASK
    return table[np.frombuffer(bytes(seq), dtype=np.uint8)]


def last_row(pmask, tmask, prefix):
    """D[m][0 .. n] of the pattern's masks (rows) against the text's (columns); top row j (prefix) or 0"""
    m, n = len(pmask), len(tmask)
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    out = np.empty(n + 1, dtype=np.int64)
    out[0] = m
    new = np.empty(m + 1, dtype=np.int64)
    for j in range(1, n + 1):
        new[0] = j if prefix else 0
        np.minimum(col[1:] + 1, col[:-1] + ((pmask & tmask[j - 1]) == 0), out=new[1:])
        col = np.minimum.accumulate(new - idx) + idx
        out[j] = col[m]
    return out


_ROWS = {}


def row_of(pattern, text, mode, flag):
    key = (pattern, text, mode, flag)
    if key not in _ROWS:
        _ROWS[key] = last_row(masks(pattern, "p", flag), masks(text, "t", flag), mode == PREFIX)[1:]
    return _ROWS[key]


def start_of(pattern, text, e, score, flag):
    """the smallest s for which the global distance of the pattern against text[s:e] is `score`, on the last min(e, m + score)
    columns (no stretch is longer)"""
    w = min(e, len(pattern) + score)
    back = last_row(masks(pattern, "p", flag)[::-1], masks(text, "t", flag)[e - w:e][::-1], True)[1:]
    assert int(back.min()) == score, (len(pattern), e, score, int(back.min()))
    return e - (int(np.nonzero(back == score)[0][-1]) + 1)


_LOC = {}


def locate(pattern, text, mode, flag):
    """-> (d, text_start, text_end) without a bound"""
    key = (pattern, text, mode, flag)
    if key not in _LOC:
        row = row_of(pattern, text, mode, flag)
        d = int(row.min())
        end = int(np.argmax(row == d)) + 1
        _LOC[key] = (d, 0 if mode == PREFIX else start_of(pattern, text, end, d, flag), end)
    return _LOC[key]


bounded = S.bounded


def occurrences(pattern, text, mode, flag, bound):
    """-> [(text_start, text_end, score)] ordered by text_end"""
    k = min(int(bound), len(pattern))
    return [(0 if mode == PREFIX else start_of(pattern, text, e, v, flag), e, v) for e, v in H.valleys(row_of(pattern, text, mode, flag), k)]


# ---- edlib ------------------------------------------------------------------------------------------------------------
class EqualityPair(C.Structure):
    _fields_ = [("first", C.c_char), ("second", C.c_char)]


def equality_pairs():
    """the unordered pairs of distinct letters of LETTERS whose sets intersect"""
    return [(a, b) for i, a in enumerate(LETTERS) for b in LETTERS[i + 1:] if set(SETS[a]) & set(SETS[b])]


_PAIRS = None


def edlib_locate(pattern, text, mode):
    """as search_lib.edlib_locate, with the IUPAC equalities: [d, startLocations[0], endLocations[0] + 1] (end location -1
    comes back as 0)"""
    global _PAIRS
    if S._edlib is None:
        S.edlib_locate(b"A", b"A", INFIX)         # loads the library and sets the prototypes
    if _PAIRS is None:
        pairs = equality_pairs()
        assert len(pairs) == 80
        _PAIRS = (EqualityPair * len(pairs))(*[EqualityPair(a.encode(), b.encode()) for a, b in pairs])
    cfg = S.EdlibAlignConfig(-1, S.EDLIB_MODE[mode], S.EDLIB_TASK_LOC, C.cast(_PAIRS, C.c_void_p), len(_PAIRS))
    r = S._edlib.edlibAlign(bytes(pattern), len(pattern), bytes(text), len(text), cfg)
    assert r.status == 0 and r.numLocations >= 1
    out = [int(r.editDistance), int(r.startLocations[0]), int(r.endLocations[0]) + 1]
    S._edlib.edlibFreeAlignResult(r)
    return out


def edlib_judges(pattern, text, flag):
    """is edlib an opinion on this case?  upper-case input over the 15 letters under IUPAC; under IUPAC_PATTERN only where the
    text is upper-case ACGT (then both flags mean the same)"""
    ok = set(LETTERS.encode())
    if not (set(pattern) <= ok and set(text) <= ok):
        return False
    return flag == IUPAC or set(text) <= set(b"ACGT")
