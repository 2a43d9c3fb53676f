"""Alignment tags (quicked_batch_configure_tags) restated in Python, for the CPU and GPU tests: the statistics and the MD:Z
string as functions of an alignment's operation sequence and the pattern's raw bytes (include/quicked_batch.h).  I consumes
text, D consumes pattern; runs are maximal.  Nothing here comes from the library."""
import re

import numpy as np

M, X, I, D = 0, 1, 2, 3
OPS = {"M": M, "X": X, "I": I, "D": D}
NONE_STATS = (-1,) * 8
_RUN = re.compile(r"(\d+)([MXID])")


def parse_cigar(cigar):
    """a style-0 CIGAR ("12M1X3I") -> [(op, len)]"""
    runs = [(OPS[o], int(n)) for n, o in _RUN.findall(cigar)]
    assert "".join(f"{n}{'MXID'[o]}" for o, n in runs) == cigar, cigar
    return runs


def merge(ops):
    """maximal runs: zero-length entries dropped, equal neighbours joined"""
    out = []
    for o, n in ops:
        if n <= 0:
            continue
        if out and out[-1][0] == o:
            out[-1][1] += n
        else:
            out.append([o, n])
    return out


def stats(ops):
    """(matches, mismatches, ins_bases, del_bases, ins_runs, del_runs, longest_match, columns)"""
    runs = merge(ops)
    tot = [sum(n for o, n in runs if o == k) for k in range(4)]
    return (tot[M], tot[X], tot[I], tot[D], sum(1 for o, _ in runs if o == I), sum(1 for o, _ in runs if o == D),
            max([n for o, n in runs if o == M], default=0), sum(tot))


def md(ops, pattern):
    """the MD:Z string; `pattern` = bytes.  -> bytes (the pattern's bytes are raw: they need not be text)"""
    out, acc, v = bytearray(), 0, 0
    for o, n in merge(ops):
        if o == M:
            acc += n
            v += n
        elif o == X:
            for _ in range(n):
                out += b"%d" % acc
                out.append(pattern[v])
                acc, v = 0, v + 1
        elif o == D:
            out += b"%d^" % acc
            out += pattern[v:v + n]
            acc, v = 0, v + n
    out += b"%d" % acc
    assert v == len(pattern) or not ops, (v, len(pattern))
    return bytes(out)


def md_bound(m):
    """what the library reserves per pair: the string and its terminator"""
    return 3 * m + 11


def expected_from_cigars(pairs, cigars):
    """per pair (stats tuple, MD str or None) from the style-0 CIGARs of a run (None: no alignment)"""
    out = []
    for (p, _), c in zip(pairs, cigars):
        if c is None:
            out.append((NONE_STATS, None))
        else:
            ops = parse_cigar(c)
            out.append((stats(ops), md(ops, p).decode("latin-1")))
    return out


def identities_hold(st, m, n, score):
    mt, mm, ib, db = st[:4]
    return mt + mm + db == m and mt + mm + ib == n and mm + ib + db == score and st[7] == mt + mm + ib + db


def n_runs(cigar):
    return len(_RUN.findall(cigar))


def mutate(rng, seq, error):
    """substitutions, insertions and deletions at rate `error` over ACGT"""
    out = bytearray()
    for b in seq:
        r = rng.random()
        if r < error / 3:
            out.append(rng.choice([c for c in b"ACGT" if c != b]))
        elif r < 2 * error / 3:
            out.append(b)
            out.append(int(rng.choice(list(b"ACGT"))))
        elif r < error:
            continue
        else:
            out.append(b)
    return bytes(out)


def random_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tolist())
