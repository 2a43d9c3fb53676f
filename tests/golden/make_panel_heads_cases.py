"""Writes tests/golden/panel_heads_cases.json: the cases of the 5' heads (QUICKED_PANEL_HEADS) with the answers of the definition
(tests/panel_heads_lib.py: the tails of the reversed texts against the reversed members, from the full matrix, in Python).  Run
it from the repository root:

    python tests/golden/make_panel_heads_cases.py

Two sets, each a list of groups {name, panel, bounds, texts, heads}; heads holds, per "flag:min_overlap" (flags 0, IUPAC 16,
IUPAC_PATTERN 32; min_overlap 1 and 3), one [pattern, overlap, text_end, score] per text.

named   groups built for what can go wrong, every construction asserted below against the definition:
        lengths, adapters, whole_bound, tall, iupac
                   the groups of make_panel_tails_cases.py mirrored -- every member and every text reversed --, so that what was
                   built at a text's end sits at its start; that generator asserts the constructions on its side of the mirror
                   and this one asserts the mirror: members of 1 .. 256 bases in all three block forms, heads on a block's last
                   row (64, 128), k = 0 and k = m, r k / m at a step, r against r + 1, 3 exact bases against 20 with one error,
                   equal keys in two members, live blocks that stop short of the last block, a text N under each flag, texts
                   shorter than the overlap, an empty text
        edges      the issue's hand case; heads at r = m - 1; texts of 63, 64, 65 and 128 bases; a text shorter than its head's
                   overlap; a full occurrence, a tail and a head in one text
        long       texts of 300 .. 5 000 bases against members whose reach m + k is 64, 65, 127, 128, 100, 192 and 263: the sweep
                   stops before the text does and its partial first chunk has every shift class (reach mod 64 in {0, 1, 63, other})
random  the random groups of that generator mirrored: mutated suffixes of the members planted at the start of half the texts,
        ACGT and IUPAC letters; between a third and two thirds of the texts have a head (asserted here and by
        tests/test_panel_heads_cpu.py)
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import panel_heads_lib as H  # noqa: E402
import panel_tails_lib as T  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_panel_tails_cases", os.path.join(HERE, "make_panel_tails_cases.py"))
GT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GT)

PATH = os.path.join(HERE, "panel_heads_cases.json")
FLAGS = GT.FLAGS
OVERLAPS = GT.OVERLAPS
rand_seq, mutate = GT.rand_seq, GT.mutate


def group(name, panel, bounds, texts):
    g = {"name": name, "panel": [bytes(p) for p in panel], "bounds": [int(b) for b in bounds], "texts": [bytes(t) for t in texts]}
    g["heads"] = {(f, mo): H.all_heads(g["texts"], g["panel"], g["bounds"], f, mo) for f in FLAGS for mo in OVERLAPS}
    return g


def mirror(tg):
    """a group of the tails' generator, every sequence reversed: its tails are this group's heads, text_end = n - text_start"""
    g = group(tg["name"], [p[::-1] for p in tg["panel"]], tg["bounds"], [t[::-1] for t in tg["texts"]])
    for key, tails in tg["tails"].items():
        want = [t if t == T.NONE else (t[0], t[1], len(x) - t[2], t[3]) for t, x in zip(tails, tg["texts"])]
        assert g["heads"][key] == want, (tg["name"], key)
    return g


def start_with(rng, head, n):
    """a text of n bases that begins with `head` (cut at the back if it is longer)"""
    return (head + rand_seq(rng, max(0, n - len(head))))[:n]


def edges_group(rng):
    a = b"AGATCGGAAGAGC"
    b = rand_seq(rng, 70)
    c = rand_seq(rng, 130)
    panel = [a, b, c]
    bounds = [1, 5, 9]
    texts = [
        b"TCGGAAGAGCCTCTCTCT",                                # 0  the hand case
        b"CTCTCTCT",                                          # 1  ... and no head
        start_with(rng, a[1:], 40),                           # 2  r = m - 1 = 12
        start_with(rng, b[1:], 150),                          # 3  r = m - 1 = 69, block 1's row 5
        start_with(rng, c[1:], 150),                          # 4  r = m - 1 = 129, block 2's first row
        c[-128:],                                             # 5  n = 128 = r: block 1's last row, the whole text
        start_with(rng, c[-128:], 129),
        start_with(rng, b[-64:], 64),                         # 7  n = 64 = r
        start_with(rng, b[-64:], 65),
        start_with(rng, b[-64:], 63),                         # 9  n = 63 < 64: the head is shorter or has a deletion
        start_with(rng, mutate(rng, b[-60:], 3), 63),
        c[-100:-40],                                          # 11 n = 60 < r for every long head: the member runs past the text
        a[-10:] + rand_seq(rng, 20, "CT") + a + rand_seq(rng, 20, "CT") + a[:9],      # 12 a head, a full occurrence and a tail
    ]
    g = group("edges", panel, bounds, texts)
    h3 = g["heads"][(0, 3)]
    assert h3[0] == (0, 10, 10, 0) and h3[1] == H.NONE, (h3[0], h3[1])
    assert h3[2] == (0, 12, 12, 0) and h3[3] == (1, 69, 69, 0) and h3[4] == (2, 129, 129, 0), (h3[2], h3[3], h3[4])
    assert h3[5] == (2, 128, 128, 0) and h3[6] == (2, 128, 128, 0) and h3[7] == (1, 64, 64, 0) and h3[8] == (1, 64, 64, 0), h3[5:9]
    assert h3[9][0] == 1 and h3[9][2] == 63 and h3[9][1] - h3[9][3] <= 63, h3[9]
    assert {len(t) for t in texts} >= {63, 64, 65, 128}
    assert h3[12] == (0, 10, 10, 0), h3[12]
    assert T.text_tail(texts[12], panel, bounds, 0, 3)[:2] == (0, 9)
    assert int(T.matrix(T.equal(a, texts[12], 0))[-1].min()) == 0                         # the full occurrence
    return g


def long_group(rng):
    """reach m + k of 64, 65, 127, 128, 100, 192 and 263 columns in texts of 300 .. 5 000"""
    shapes = [(60, 4), (60, 5), (120, 7), (120, 8), (92, 8), (180, 12), (250, 13)]
    panel = [rand_seq(rng, m) for m, _ in shapes]
    bounds = [k for _, k in shapes]
    assert sorted({H.reach(q, k) % 64 for q, k in zip(panel, bounds)}) == [0, 1, 7, 36, 63]
    texts = []
    for p, (m, k) in enumerate(shapes):
        for i, n in enumerate((300, 1000, 5000)):
            r = (m - 1, m // 2, 64 if m > 64 else 20)[i]
            head = panel[p][m - r:]
            texts.append(start_with(rng, head, n))
            # as many insertions as the row allows: the stretch reaches r + d columns, the most a head of this row can
            d = (r * k) // m
            grown = bytearray(head)
            for j in range(d):
                grown.insert(3 + 2 * j, ord("ACGT"[("ACGT".index(chr(grown[3 + 2 * j])) + 1) % 4]))
            texts.append(start_with(rng, bytes(grown), n))
    texts.append(rand_seq(rng, 2000, "CT"))
    g = group("long", panel, bounds, texts)
    h3 = g["heads"][(0, 3)]
    assert all(300 <= len(t) <= 5000 for t in texts) and all(H.reach(q, k) < 300 for q, k in zip(panel, bounds))
    for p, (m, k) in enumerate(shapes):
        got = h3[6 * p:6 * p + 6]
        assert all(x[0] == p for x in got), (p, got)
        assert got[0] == (p, m - 1, m - 1, 0), got[0]
        assert got[1][1] == m - 1 and got[1][3] == ((m - 1) * k) // m and got[1][2] == m - 1 + got[1][3], (p, got[1])      # r + d = m - 1 + k at the most
    assert any(x[3] > 0 for x in h3)
    return g


def have_share(groups, key):
    heads = [t for g in groups for t in g["heads"][key]]
    return sum(t[0] >= 0 for t in heads) / len(heads)


def build():
    rng = np.random.default_rng(20261020)
    named = [mirror(GT.lengths_group(rng)), mirror(GT.adapters_group(rng)), mirror(GT.whole_bound_group(rng)), mirror(GT.tall_group(rng)),
             mirror(GT.iupac_group(rng)), edges_group(rng), long_group(rng)]
    lengths = named[0]["heads"][(0, 3)]
    assert {t[1] for t in lengths} >= {62, 63, 64, 65, 127, 128, 129}
    ad = named[1]["heads"][(0, 3)]
    assert ad[0] == (0, 12, 12, 0) and ad[8] == (0, 15, 15, 0) and ad[9][:2] == (0, 20) and ad[9][3] == 1 and ad[7] == (4, 6, 6, 1), ad
    assert ad[10][:2] == (0, 9) and ad[5] == H.NONE
    assert named[3]["heads"][(0, 3)][0] == (0, 40, 40, 0)                                   # blocks 1 .. 3 of member 0 are not live
    iu = named[4]["heads"]
    assert iu[(T.IUPAC, 1)][4][0] >= 0 and iu[(T.IUPAC_PATTERN, 1)][4] == H.NONE and iu[(0, 1)][4][0] >= 0      # a text N under each flag
    rnd = [mirror(GT.random_group(rng, "acgt", "ACGT", 120, 6)), mirror(GT.random_group(rng, "letters", "ACGTACGTACGTACGTRYN", 60, 4))]
    for f in FLAGS:
        share = have_share(rnd, (f, 3))
        print("flag", f, "share of texts with a head", round(share, 3))
        assert 1 / 3 <= share <= 2 / 3, (f, share)
    return {"named": named, "random": rnd}


def dump(sets):
    out = {}
    for name, groups in sets.items():
        out[name] = [{"name": g["name"], "panel": [p.decode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.decode() for t in g["texts"]],
                      "heads": {"%d:%d" % k: [list(t) for t in v] for k, v in g["heads"].items()}} for g in groups]
    with open(PATH, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


def load():
    with open(PATH) as f:
        raw = json.load(f)
    sets = {}
    for name, groups in raw.items():
        sets[name] = [{"name": g["name"], "panel": [p.encode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.encode() for t in g["texts"]],
                       "heads": {tuple(int(x) for x in k.split(":")): [tuple(t) for t in v] for k, v in g["heads"].items()}} for g in groups]
    return sets


if __name__ == "__main__":
    dump(build())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
