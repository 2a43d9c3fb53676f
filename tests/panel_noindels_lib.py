"""Panel search by mismatches only (QUICKED_PANEL_NO_INDELS): the definition, by plain loops over bytes.

Member p (m bases, effective bound k = min(bound, m)) against a text of n bases.  For a start s in [0, n - m], H[s] counts the
positions r in [0, m) where member[r] and text[s + r] are NOT equal under the run's equality; R[e] = H[e - m] for the ends e in E
-- INFIX {m .. n}, PREFIX {m}, none when n < m --, and every column outside E counts as higher than every value.  The best run:
d = min R, text_end the smallest e that has it, beyond where d > k.  Every occurrence: e with R[e] <= k, R[e] < R[e - 1], and the
first later e' of E with another value, if any, has a higher one.  text_start = text_end - m.

The three equalities are written out here, byte by byte, and share nothing with quicked_amd/csrc (qe_search.h, qe_iupac.h,
qe_panel_ham.h) nor with the other test libraries:
    unflagged        case is folded; A, C, G, T are themselves and every other byte is one more symbol
    IUPAC            both bytes are base sets (U = T; a byte that is no IUPAC letter is the empty set); equal = they intersect
    IUPAC_PATTERN    the member as under IUPAC; a text byte that is not one of ACGTU (either case) is the empty set

H_batch is the same count with the loop over the texts done by numpy, for the one test at size; tests/test_panel_noindels_cpu.py
holds it to the plain loops.
"""
import numpy as np

PREFIX, INFIX = 1, 2
IUPAC, IUPAC_PATTERN = 16, 32
NO_INDELS = 32768
MATRIX = 64
INT32_MAX = 2**31 - 1
HIT_FIELDS = ("pattern", "score", "text_start", "text_end", "second_pattern", "second_score")
OCC_FIELDS = ("pattern", "text_start", "text_end", "score")

_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def _plain_symbol(byte):
    c = chr(byte).upper()
    return c if c in "ACGT" else "other"


def _base_set(byte, acgtu_only):
    c = chr(byte).upper()
    if acgtu_only and c not in "ACGTU":
        return frozenset()
    return frozenset(_SETS.get(c, ""))


def differ(pb, tb, flag):
    """True where member byte pb and text byte tb are NOT equal under the run's equality"""
    if flag == 0:
        return _plain_symbol(pb) != _plain_symbol(tb)
    return not (_base_set(pb, False) & _base_set(tb, flag == IUPAC_PATTERN))


_TABLES = {}


def table(flag):
    """-> 256 rows of 256 bytes: row[pb][tb] = 1 where the two bytes differ (differ(), tabulated once per flag)"""
    if flag not in _TABLES:
        _TABLES[flag] = [bytes(1 if differ(pb, tb, flag) else 0 for tb in range(256)) for pb in range(256)]
    return _TABLES[flag]


def H_of(member, text, flag):
    """-> [H[0] .. H[n - m]] ([]: n < m)"""
    rows = [table(flag)[pb] for pb in member]
    m, n = len(member), len(text)
    out = []
    for s in range(n - m + 1):
        h = 0
        for r in range(m):
            h += rows[r][text[s + r]]
        out.append(h)
    return out


def R_of(member, text, mode, flag):
    """-> {e: R[e]} over E, in ascending order of e"""
    H = H_of(member, text, flag)
    m = len(member)
    if mode == PREFIX:
        H = H[:1]
    return {s + m: h for s, h in enumerate(H)}


def best_of(R, k):
    """-> (d, text_end) or (-1, -1): the smallest value within k and the smallest end that has it"""
    d, end = -1, -1
    for e, v in R.items():
        if v <= k and (d < 0 or v < d):
            d, end = v, e
    return d, end


def valleys_of(R, k):
    """-> [(text_end, score)]: the valley rule, written as the three conditions of the contract"""
    ends = sorted(R)
    out = []
    for i, e in enumerate(ends):
        v = R[e]
        if v > k:
            continue
        if i > 0 and not v < R[ends[i - 1]]:
            continue
        later = [R[x] for x in ends[i + 1:] if R[x] != v]
        if later and not later[0] > v:
            continue
        out.append((e, v))
    return out


def bound_of(bounds, p, member):
    return min(int(bounds[p]), len(member))


def matrix(texts, panel, bounds, mode, flag):
    """-> (D, E) lists [n][K]: every member's {d or -1, text_end or -1} in every text; an empty text's row is -1"""
    D, E = [], []
    for t in texts:
        drow, erow = [], []
        for p, q in enumerate(panel):
            d, e = best_of(R_of(q, t, mode, flag), bound_of(bounds, p, q)) if t else (-1, -1)
            drow.append(d)
            erow.append(e)
        D.append(drow)
        E.append(erow)
    return D, E


def reduce_text(drow, erow, panel):
    """one text's matrix row -> the six HIT_FIELDS by the key (score, panel index); text_start = text_end - m"""
    keys = sorted((d, p) for p, d in enumerate(drow) if d >= 0)
    if not keys:
        return (-1,) * 6
    d, p = keys[0]
    d2, p2 = keys[1] if len(keys) > 1 else (-1, -1)
    return (p, d, erow[p] - len(panel[p]), erow[p], p2, d2)


def text_hits(text, panel, bounds, mode, flag):
    """-> [(pattern, text_start, text_end, score)] of one text, ordered by (pattern, text_end), uncapped"""
    out = []
    if not text:
        return out
    for p, q in enumerate(panel):
        out += [(p, e - len(q), e, v) for e, v in valleys_of(R_of(q, text, mode, flag), bound_of(bounds, p, q))]
    return out


def capped(hits, max_hits):
    """one text's uncapped list -> (found, the stored ones, the text's score)"""
    return len(hits), hits[:max_hits], (min(o[3] for o in hits) if hits else -1)


def best_two(hits):
    """consequence 1: the smallest key with its first occurrence, and the smallest key among the other members"""
    if not hits:
        return (-1,) * 6
    key = min((o[3], o[0]) for o in hits)
    first = next(o for o in hits if (o[3], o[0]) == key)
    others = [(o[3], o[0]) for o in hits if o[0] != key[1]]
    second = min(others) if others else (-1, -1)
    return (key[1], key[0], first[1], first[2], second[1], second[0])


def member_best(hits, k):
    """consequence 2: -> (score [k], text_end [k]): every member's smallest score and the first end that has it"""
    sc, en = [-1] * k, [-1] * k
    for p, _, e, v in hits:
        if sc[p] < 0 or v < sc[p]:
            sc[p], en[p] = v, e
    return sc, en


def block_steps(texts, panel, mode):
    """counter [0]: per (text, member) the start positions x ceil(m / 64)"""
    total = 0
    for t in texts:
        for q in panel:
            n, m = len(t), len(q)
            starts = 0 if n < m else (1 if mode == PREFIX else n - m + 1)
            total += starts * ((m + 63) // 64)
    return total


def H_batch(member, texts, flag):
    """H_of for many texts at once -> int32 [len(texts), width - m + 1], -1 where s > n - m (width: the longest text)"""
    neq = np.array([list(row) for row in table(flag)], dtype=np.uint8)
    m, width = len(member), max(len(t) for t in texts)
    lens = np.array([len(t) for t in texts])
    T = np.zeros((len(texts), max(width, m)), dtype=np.uint8)
    for i, t in enumerate(texts):
        T[i, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    ns = T.shape[1] - m + 1
    out = np.zeros((len(texts), ns), dtype=np.int32)
    for r, pb in enumerate(member):
        out += neq[pb][T[:, r:r + ns]]
    out[np.arange(ns)[None, :] > (lens - m)[:, None]] = -1
    return out


def results_of(texts, panel, bounds, cap):
    """-> {(mode, flag): {"d", "e", "found", "occ"}} as the fixture records them: the matrix and per text its first `cap` occurrences"""
    out = {}
    for mode in (PREFIX, INFIX):
        for flag in (0, IUPAC, IUPAC_PATTERN):
            D, E = matrix(texts, panel, bounds, mode, flag)
            hits = [text_hits(t, panel, bounds, mode, flag) for t in texts]
            out[(mode, flag)] = {"d": D, "e": E, "found": [len(h) for h in hits], "occ": [h[:cap] for h in hits]}
    return out


def cases_file(path, groups, cap, flags=(0, IUPAC, IUPAC_PATTERN)):
    """the input of the native programs (tests/native/panel_noindels_cpu.cpp, panel_noindels_host.cpp): "ngroups cap", then per
    group "K n nconf", K x {member bound}, n x text ("." = empty) and per (mode, flag) "mode flag" and n x {K scores, K ends,
    found, min(found, cap) x {pattern text_start text_end score}} as this module defines them"""
    lines = ["%d %d" % (len(groups), cap)]
    for g in groups:
        confs = [k for k in sorted(g["results"]) if k[1] in flags]
        lines.append("%d %d %d" % (len(g["panel"]), len(g["texts"]), len(confs)))
        lines += ["%s %d" % (q.decode(), b) for q, b in zip(g["panel"], g["bounds"])]
        lines += [t.decode() or "." for t in g["texts"]]
        for mode, flag in confs:
            r = g["results"][(mode, flag)]
            lines.append("%d %d" % (mode, flag))
            for i in range(len(g["texts"])):
                occ = r["occ"][i][:cap]
                assert len(occ) == min(r["found"][i], cap)
                lines.append(" ".join(str(int(v)) for v in list(r["d"][i]) + list(r["e"][i]) + [r["found"][i]] + [x for o in occ for x in o]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
