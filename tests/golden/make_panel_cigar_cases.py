"""The cases of the occurrence alignments (QUICKED_PANEL_CIGARS; tests/test_panel_cigar_cpu.py, tests/test_host_panel_cigar.py,
tests/test_gpu_panel_cigar.py) and the recorder of the definition's answers to them.

Two sets, "named" (recorded under the members' own bounds) and "random" (under those and under a uniform bound), in the format of
make_panel_hits_cases.py's sets (texts, panel, the members' own bounds, a uniform bound, per (mode, flag, own / uniform) every
text's occurrences from tests/panel_hits_lib.py) with, beside every occurrence list,
the style-0 strings of tests/panel_cigar_lib.py under "cigars".  Everything is regenerated from a seed; the generator asserts,
from the brute force and the definition alone, that the named set holds what it is for:

  lengths        members of 1, 63, 64, 65, 128, 129, 255 and 256 bases; stretches of 63, 64, 65, 127, 128 and 129 columns
  scores         d = 0; d = m with the bound clamped to m
  long runs      a deletion run over rows 62 .. 66, an insertion run over columns 62 .. 66, one of each over 126 .. 130
  ties           homopolymers (AAAA in AAA) and dinucleotide repeats, which only the D > I > diagonal order decides
  edges          an occurrence at text_start 0 that begins with D; one that ends at the text's end; an empty text
  several        two occurrences of one member and occurrences of two members in one text; a text with more than 64 occurrences
  equalities     R / Y / N members under both flags; a text N under each flag (M under IUPAC, X under IUPAC_PATTERN); lower-case
                 and N / other bytes unflagged

and, on every occurrence whose member and stretch are upper-case ACGT, that the definition's operations are the oracle's
qo_banded_align(member, stretch, cutoff = d).  Recorded in tests/golden/panel_cigar_cases.json; nothing here comes from the
library.

    python tests/golden/make_panel_cigar_cases.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as O           # noqa: E402
import panel_cigar_lib as PC     # noqa: E402
import panel_hits_lib as PH      # noqa: E402

FIXTURE = os.path.join(HERE, "panel_cigar_cases.json")
SEED = 20261020
ACGT = b"ACGT"
MODES = (PH.PREFIX, PH.INFIX)
FLAGS = (0, PH.IUPAC, PH.IUPAC_PATTERN)
CONFS = ("own", "uniform")
SET_CONFS = {"named": ("own",), "random": CONFS}      # the named set is recorded under its members' own bounds only


def rand(rng, n, letters=ACGT):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), n))


def bounds_of(s, conf):
    return s["bounds"] if conf == "own" else [s["uniform"]] * len(s["panel"])


def other(c):
    return next(x for x in ACGT if x != c)


def oracle_ops(member, stretch, d):
    buf = C.create_string_buffer(len(member) + len(stretch) + 8)
    score = C.c_int64(-1)
    a, b = C.c_int64(0), C.c_int64(0)
    n = O.oracle().qo_banded_align(member, len(member), stretch, len(stretch), d, buf, C.byref(score), C.byref(a), C.byref(b))
    return int(score.value), buf.raw[:n].decode()


class Retry(Exception):
    """random bases around a planted run let the rule split it: the next seed"""


def named_set():
    for attempt in range(64):
        try:
            return named_set_of(SEED + 100 * attempt)
        except Retry:
            continue
    raise AssertionError("no seed gives the long runs")


def named_set_of(seed):
    rng = np.random.default_rng(seed)
    # (the 1-base member and the one of d = m are N: a base would occur in every few columns of every text and fill the record)
    sized = [b"N"] + [rand(rng, n) for n in (63, 64, 65, 128, 129, 255, 256)]
    deg = bytearray(rand(rng, 19)); deg[3] = ord("Y"); deg[8] = ord("M"); deg[12] = ord("N"); deg[16] = ord("R")
    base = bytes(deg).replace(b"Y", b"C").replace(b"M", b"A").replace(b"N", b"G").replace(b"R", b"G")
    panel = sized + [b"AAAA", b"ACACAC", bytes(deg), rand(rng, 24), b"N" * 3]
    #         N  63 64 65 128 129 255 256 AAAA ACACAC deg 24  NNN
    bounds = [3, 2, 2, 2, 6, 3, 6, 4, 1, 2, 2, 3, 9]
    P1, P63, P64, P65, P128, P129, P255, P256, PA, PAC, PDEG, P24, PG = range(13)
    texts, marks = [], {}

    def add(t, mark=None):
        if mark:
            marks.setdefault(mark, []).append(len(texts))
        texts.append(bytes(t))

    def cut(q, at, n):
        return q[:at] + q[at + n:]

    def ins(q, at, n):
        fill = bytes(other(q[at]) if other(q[at]) != q[at - 1] else next(x for x in ACGT if x not in (q[at], q[at - 1])) for _ in range(n))
        return q[:at] + fill + q[at:]

    # ---- exact plants of every sized member (d = 0), in the middle (INFIX) and at the text's start (PREFIX)
    for p in range(1, 8):
        add(rand(rng, 20) + panel[p] + rand(rng, 20), "exact")
        add(panel[p] + rand(rng, 10), "exact")
    # ---- stretches of 63, 64, 65 / 127, 128, 129 columns: one base of the member missing, none, one more
    for p in (P64, P128):
        q = panel[p]
        for t in (cut(q, 30, 1), q, ins(q, 30, 1)):
            add(rand(rng, 17) + t + rand(rng, 9), "stretch")
            add(t + rand(rng, 9), "stretch")
    # ---- long runs: rows 62 .. 66 deleted, five columns inserted before column 62; the same over 126 .. 130
    add(rand(rng, 11) + cut(panel[P128], 61, 5) + rand(rng, 11), "del62")
    add(rand(rng, 11) + ins(panel[P128], 61, 5) + rand(rng, 11), "ins62")
    add(rand(rng, 11) + cut(panel[P255], 125, 5) + rand(rng, 11), "del126")
    add(rand(rng, 11) + ins(panel[P255], 125, 5) + rand(rng, 11), "ins126")
    add(cut(panel[P128], 61, 5) + rand(rng, 11), "del62")
    add(ins(panel[P255], 125, 5) + rand(rng, 11), "ins126")
    # ---- ties
    add(b"CCAAACC", "homopolymer")
    add(b"AAA", "homopolymer")
    add(b"CTAAAAAAAAACT", "homopolymer")
    add(b"GGACACGG", "dinucleotide")
    add(b"TTACACACACACTT", "dinucleotide")
    add(b"CACACA", "dinucleotide")
    # ---- d = m, the bound clamped: NNN (bound 9) against bases, unflagged
    add(b"ACAC", "d_is_m")
    # ---- a first base that is missing at text_start 0; an occurrence that ends at the text's end
    add(panel[P24][1:] + rand(rng, 12), "leading_d")
    add(rand(rng, 30) + panel[P24], "at_end")
    # ---- several occurrences: twice member 24, once member 63 and the degenerate one's expansion; many in one text
    add(rand(rng, 9) + panel[P24] + rand(rng, 15) + panel[P24][:11] + b"T" + panel[P24][12:] + rand(rng, 7) + panel[P63] + base, "several")
    add(b"AAAATTTTT" * 66, "many")
    add(b"", "empty")
    # ---- equalities: the degenerate member's expansion and a second one; a text N inside a plant; lower case and other bytes
    add(rand(rng, 14) + base + rand(rng, 14), "iupac")
    add(rand(rng, 6) + bytes(deg).replace(b"Y", b"T").replace(b"M", b"C").replace(b"N", b"T").replace(b"R", b"A") + rand(rng, 6), "iupac")
    add(rand(rng, 8) + panel[P24][:10] + b"N" + panel[P24][11:] + rand(rng, 8), "text_n")
    add(rand(rng, 8) + base[:5] + b"N" + base[6:] + rand(rng, 8), "text_n")
    add(rand(rng, 8).lower() + panel[P24].lower() + rand(rng, 8), "lower")
    add(rand(rng, 8) + panel[P24][:7] + b"n" + panel[P24][8:15] + b"-" + panel[P24][16:] + b"NN*", "other")
    s = {"texts": texts, "panel": panel, "bounds": bounds, "uniform": 3}
    attach(s, SET_CONFS["named"])
    # ---- what the set is for
    own = s["hits"][(PH.INFIX, 0, "own")]
    cig = s["cigars"][(PH.INFIX, 0, "own")]
    pre = s["hits"][(PH.PREFIX, 0, "own")]
    every = [(i, o, c) for i, (h, cs) in enumerate(zip(own, cig)) for o, c in zip(h, cs)]
    census = {}
    assert {len(q) for q in panel} >= {1, 63, 64, 65, 128, 129, 255, 256}
    assert {o[2] - o[1] for _, o, _ in every} >= {63, 64, 65, 127, 128, 129}
    for p in range(1, 8):
        assert any(o[0] == p and o[3] == 0 and c == "%dM" % len(panel[p]) for _, o, c in every), p
        assert any(o[0] == p and o[3] == 0 for h in pre for o in h), p
    assert any(o[0] == PG and o[3] == 3 and o[3] == len(panel[PG]) < bounds[PG] for i, o, c in every if i in marks["d_is_m"])

    def run_at(c, letter, first, n):
        """the string has a run of n `letter` whose first row (D) / column (I) is `first` (1-based)"""
        row = col = 0
        import re
        for k, o in re.findall(r"(\d+)([MXID])", c):
            k = int(k)
            if o == letter and k == n and (row if letter == "D" else col) + 1 == first:
                return True
            row += k if o in "MXD" else 0
            col += k if o in "MXI" else 0
        return False

    for mark, p, letter, first in (("del62", P128, "D", 62), ("ins62", P128, "I", 62), ("del126", P255, "D", 126), ("ins126", P255, "I", 126)):
        got = [c for i, o, c in every if i in marks[mark] and o[0] == p]
        if not (got and all(run_at(c, letter, first, 5) for c in got)):
            raise Retry()
        census[mark] = len(got)
    assert any(o[0] == PA and c in ("1D3M", "3M1D", "1M1D2M", "2M1D1M") for i, o, c in every if texts[i] == b"AAA")
    census["homopolymer"] = sorted({c for i, o, c in every if i in marks["homopolymer"] and o[0] == PA})
    census["dinucleotide"] = sorted({c for i, o, c in every if i in marks["dinucleotide"] and o[0] == PAC})
    assert len(census["homopolymer"]) >= 2 and len(census["dinucleotide"]) >= 2
    assert any(o[0] == P24 and o[1] == 0 and c.startswith("1D") for i, o, c in every if i in marks["leading_d"]), [x for x in every if x[0] in marks["leading_d"]]
    assert any(o[0] == P24 and o[2] == len(texts[i]) for i, o, c in every if i in marks["at_end"])
    i = marks["several"][0]
    assert sum(1 for o in own[i] if o[0] == P24) >= 2 and {o[0] for o in own[i]} >= {P24, P63}
    assert max(len(h) for h in own) > 64 and own[marks["empty"][0]] == []
    fl = {f: list(zip(s["hits"][(PH.INFIX, f, "own")], s["cigars"][(PH.INFIX, f, "own")])) for f in FLAGS}
    for i in marks["iupac"]:
        for f in (PH.IUPAC, PH.IUPAC_PATTERN):
            assert any(o[0] == PDEG and o[3] == 0 and c == "19M" for o, c in zip(*fl[f][i])), (i, f)
        assert not any(o[0] == PDEG and o[3] == 0 for o in fl[0][i][0])
    i = marks["text_n"][0]                          # a text N: a base set under IUPAC, the empty set under IUPAC_PATTERN, a symbol of its own unflagged
    assert any(o[0] == P24 and c == "24M" for o, c in zip(*fl[PH.IUPAC][i]))
    assert any(o[0] == P24 and c == "10M1X13M" for o, c in zip(*fl[PH.IUPAC_PATTERN][i]))
    assert any(o[0] == P24 and c == "10M1X13M" for o, c in zip(*fl[0][i]))
    i = marks["text_n"][1]
    assert any(o[0] == PDEG and c == "19M" for o, c in zip(*fl[PH.IUPAC][i])) and any(o[0] == PDEG and c == "5M1X13M" for o, c in zip(*fl[PH.IUPAC_PATTERN][i]))
    assert any(o[0] == P24 and c == "24M" for o, c in zip(*fl[0][marks["lower"][0]]))
    assert any(o[0] == P24 and c == "7M1X7M1X8M" for o, c in zip(*fl[0][marks["other"][0]]))
    s["census"] = census
    return s


def random_set():
    rng = np.random.default_rng(SEED + 1)
    panel = [rand(rng, n) for n in (12, 24, 31, 64, 70, 130)]
    deg = bytearray(panel[1]); deg[4] = ord("R"); deg[17] = ord("N")
    panel.append(bytes(deg))
    bounds = [2, 4, 5, 6, 9, 12, 3]
    texts = []
    for _ in range(36):
        t = bytearray(rand(rng, int(rng.integers(30, 260))))
        for _ in range(int(rng.integers(1, 4))):
            q = bytearray(panel[int(rng.integers(0, len(panel)))].replace(b"R", b"A").replace(b"N", b"C"))
            for _ in range(int(rng.integers(0, 1 + len(q) // 8))):
                at, how = int(rng.integers(0, len(q))), int(rng.integers(0, 3))
                if how == 0:
                    q[at] = ACGT[int(rng.integers(0, 4))]
                elif how == 1:
                    del q[at]
                else:
                    q.insert(at, ACGT[int(rng.integers(0, 4))])
            at = int(rng.integers(0, len(t) + 1))
            t[at:at] = q
        if rng.integers(0, 4) == 0:
            t[int(rng.integers(0, len(t)))] = ord("N")
        texts.append(bytes(t))
    s = {"texts": texts, "panel": panel, "bounds": bounds, "uniform": 4}
    attach(s)
    s["census"] = {"occurrences": sum(len(h) for h in s["hits"][(PH.INFIX, 0, "own")])}
    return s


def attach(s, confs=CONFS):
    """the set's occurrence lists and their strings, and the oracle's opinion where it has one"""
    s["hits"], s["cigars"] = {}, {}
    judged = 0
    for mode in MODES:
        for conf in confs:
            for flag in FLAGS:
                hits = PH.all_hits(s["texts"], s["panel"], bounds_of(s, conf), mode, flag)
                cigs = [PC.hit_cigars(t, s["panel"], h, flag) for t, h in zip(s["texts"], hits)]
                s["hits"][(mode, flag, conf)], s["cigars"][(mode, flag, conf)] = hits, cigs
                for t, h, cs in zip(s["texts"], hits, cigs):
                    for (p, a, e, v), c in zip(h, cs):
                        PC.invariants(c, 0, len(s["panel"][p]), e - a, v, mode == PH.PREFIX)
                        if flag == 0 and set(s["panel"][p]) <= set(ACGT) and set(t[a:e]) <= set(ACGT):
                            d, ops = oracle_ops(s["panel"][p], t[a:e], v)
                            assert d == v and PC.rle(ops) == c, (p, a, e, v, d, PC.rle(ops), c)
                            judged += 1
    assert judged > 50
    s["judged"] = judged


def flat(s):
    """under a flag, null where a text's list (and its strings) is that of the flag before it in FLAGS (IUPAC: the unflagged one;
    IUPAC_PATTERN: IUPAC's -- they differ only where a text has a byte that is not ACGT)"""
    hits, cigs = {}, {}
    for (mode, flag, conf), v in s["hits"].items():
        h = [[int(x) for o in t for x in o] for t in v]
        c = s["cigars"][(mode, flag, conf)]
        if flag:
            before = (mode, FLAGS[FLAGS.index(flag) - 1], conf)
            same = [a == b and x == y for a, b, x, y in zip(v, s["hits"][before], c, s["cigars"][before])]
            h, c = [None if q else t for t, q in zip(h, same)], [None if q else t for t, q in zip(c, same)]
        hits["%d_%d_%s" % (mode, flag, conf)], cigs["%d_%d_%s" % (mode, flag, conf)] = h, c
    return {"texts": [t.decode() for t in s["texts"]], "panel": [q.decode() for q in s["panel"]], "bounds": s["bounds"], "uniform": s["uniform"],
            "hits": hits, "cigars": cigs, "census": s["census"], "judged": s["judged"]}


def load():
    """-> {"named": set, "random": set}: the lists under "hits"[(mode, flag, "own" / "uniform")], their strings under "cigars" """
    with open(FIXTURE) as f:
        raw = json.load(f)
    out = {}
    for name in ("named", "random"):
        s = raw[name]
        hits, cigs, raw_h, raw_c = {}, {}, {}, {}
        for k in sorted(s["hits"], key=lambda k: int(k.split("_")[1])):              # a flag's nulls are filled from the flag before it
            mode, flag, conf = k.split("_")
            before = "%s_%d_%s" % (mode, FLAGS[FLAGS.index(int(flag)) - 1], conf)
            raw_h[k] = [raw_h[before][i] if h is None else h for i, h in enumerate(s["hits"][k])]
            raw_c[k] = [raw_c[before][i] if x is None else x for i, x in enumerate(s["cigars"][k])]
            hits[(int(mode), int(flag), conf)] = [[tuple(h[i:i + 4]) for i in range(0, len(h), 4)] for h in raw_h[k]]
            cigs[(int(mode), int(flag), conf)] = raw_c[k]
        out[name] = {"texts": [t.encode() for t in s["texts"]], "panel": [q.encode() for q in s["panel"]], "bounds": s["bounds"], "uniform": s["uniform"],
                     "hits": hits, "cigars": cigs}
    return out


def main():
    doc = {"seed": SEED, "named": flat(named_set()), "random": flat(random_set())}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes", doc["named"]["census"], doc["named"]["judged"], doc["random"]["census"], doc["random"]["judged"])
    assert os.path.getsize(FIXTURE) <= 1 << 20


if __name__ == "__main__":
    main()
