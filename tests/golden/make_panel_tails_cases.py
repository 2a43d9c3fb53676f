"""Writes tests/golden/panel_tails_cases.json: the cases of the 3' tails (QUICKED_PANEL_TAILS) with the answers of the definition
(tests/panel_tails_lib.py: the full matrix and the rule, in Python).  Run it from the repository root:

    python tests/golden/make_panel_tails_cases.py

Two sets, each a list of groups {name, panel, bounds, texts, tails}; tails holds, per "flag:min_overlap" (flags 0, IUPAC 16,
IUPAC_PATTERN 32; min_overlap 1 and 3), one [pattern, overlap, text_start, score] per text.

named   groups built for what can go wrong, every construction asserted below against the definition:
        lengths    members of 1, 2, 3, 63, 64, 65, 128, 129 and 256 bases (all three block forms; tails that end exactly on a
                   block's last row: rows 64 and 128) in texts of 1, 2, 63, 64, 65 and 150 bases
        adapters   24-base members: k = 0, r k / m exactly at a step, an exact tail at r beside the one-deletion tail at r + 1,
                   a 3-base chance match beside a 20-base tail with one error, two members with equal keys, a full occurrence
                   and a tail in one text, texts shorter than min_overlap, an empty text
        whole_bound  k = m: a text shorter than the tail's overlap, whose score is then all deletions
        tall       a 256-base member with a small bound whose tail lies in block 0 while blocks 1 .. 3 are not live, and tails
                   deep in blocks 1, 2 and 3 of members with wide bounds
        iupac      degenerate letters in the members, N and other letters in the texts: the three flags disagree
random  mutated prefixes of the members planted at the end of half the texts, ACGT and IUPAC letters; between a third and two
        thirds of the texts have a tail (asserted here and by tests/test_panel_tails_cpu.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import panel_tails_lib as T  # noqa: E402

PATH = os.path.join(HERE, "panel_tails_cases.json")
FLAGS = (0, T.IUPAC, T.IUPAC_PATTERN)
OVERLAPS = (1, 3)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(c)] for c in rng.integers(0, len(alphabet), n)).encode()


def mutate(rng, s, edits):
    """`edits` random substitutions, insertions and deletions, none at the last base"""
    s = bytearray(s)
    for _ in range(edits):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, max(1, len(s) - 1)))
        if kind == 0:
            s[at] = ord("ACGT"[("ACGT".index(chr(s[at])) + 1 + int(rng.integers(0, 3))) % 4]) if chr(s[at]) in "ACGT" else ord("A")
        elif kind == 1:
            s.insert(at, ord("ACGT"[int(rng.integers(0, 4))]))
        elif len(s) > 1:
            del s[at]
    return bytes(s)


def group(name, panel, bounds, texts):
    g = {"name": name, "panel": [bytes(p) for p in panel], "bounds": [int(b) for b in bounds], "texts": [bytes(t) for t in texts]}
    g["tails"] = {(f, mo): T.all_tails(g["texts"], g["panel"], g["bounds"], f, mo) for f in FLAGS for mo in OVERLAPS}
    return g


def fit(rng, tail, n):
    """a text of n bases that ends with `tail` (cut at the front if it is longer)"""
    return (rand_seq(rng, max(0, n - len(tail))) + tail)[-n:]


def lengths_group(rng):
    lens = (1, 2, 3, 63, 64, 65, 128, 129, 256)
    panel = [rand_seq(rng, m) for m in lens]
    bounds = [0, 1, 1, 6, 6, 6, 12, 13, 25]
    texts = [panel[1][:1], panel[2][:2], b"", b"G"]
    for p, m in enumerate(lens):
        for r in sorted({1, 2, 3, 20, 62, 63, 64, 65, 127, 128, 129, 255, m - 1}):
            if r >= m or r < 1:
                continue
            for n in (63, 64, 65, 150):
                clean = panel[p][:r]
                texts.append(fit(rng, clean, n))
                if r >= 20:
                    texts.append(fit(rng, mutate(rng, clean, (r * min(bounds[p], m)) // m), n))
    g = group("lengths", panel, bounds, texts)
    tails = g["tails"][(0, 3)]
    assert {len(t) for t in texts} >= {0, 1, 2, 63, 64, 65, 150}
    assert {t[1] for t in tails} >= {62, 63, 64, 65, 127, 128, 129}, sorted({t[1] for t in tails})
    assert {t[0] for t in tails} >= {3, 4, 5, 6, 7, 8}
    assert any(t[3] > 0 for t in tails) and any(t == T.NONE for t in tails)
    return g


def adapters_group(rng):
    a = b"AGATCGGAAGAGCACACGTCTGAA"                     # 24 bases each
    b = b"CTGTCTCTTATACACATCTCCGAG"
    mut = bytearray(a[:20])
    mut[9] = ord("T") if mut[9] != ord("T") else ord("C")
    mut = bytes(mut)
    d = mut[-3:] + b"CCCCCCCCCCCCCCCCCCCCC"               # begins with the last three bases of the mutated tail of `a`
    e = b"GGTTCCAAGGTTCCAAGGTTCCAA"
    panel = [a, b, d, a, e]
    bounds = [4, 0, 4, 4, 4]
    five = bytearray(e[:5]); five[1] = ord("A")            # r k / m at a step: row 5 of `e` allows floor(5 * 4 / 24) = 0 ...
    six = bytearray(e[:6]); six[1] = ord("A")              # ... and row 6 allows 1
    texts = [
        rand_seq(rng, 40, "CT") + b"TTTT" + a[:12],          # 0  a plain tail; members 0 and 3 have equal keys: 0 wins
        rand_seq(rng, 40, "AG") + b[:10],                    # 1  k = 0: the exact prefix is a tail
        rand_seq(rng, 40, "AG") + b[:5] + b"A" + b[6:12],    # 2  k = 0: one error is none (b[5] is C)
        b"AG",                                               # 3  shorter than min_overlap 3
        b"G",                                                # 4  one base
        b"",                                                 # 5  empty
        b"CCCCCCCC" + bytes(five),                           # 6  5 bases with one error: not a tail of `e`
        b"CCCCCCCC" + bytes(six),                            # 7  6 bases with one error: a tail of `e`
        b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTT" + a[:15],          # 8  exact at r = 15 beside one deletion at r = 16: 15 wins
        rand_seq(rng, 30, "CT") + mut,                       # 9  20 bases of `a` with one error end in three bases of `d`: `a` wins
        rand_seq(rng, 20, "CT") + a + rand_seq(rng, 30, "CT") + a[:9],      # 10 a full occurrence and a tail
        rand_seq(rng, 20, "AG") + b + b"A",                  # 11 a full occurrence (k = 0) and no tail of it
        rand_seq(rng, 150, "CT"),                            # 12 nothing
    ]
    g = group("adapters", panel, bounds, texts)
    t1, t3 = g["tails"][(0, 1)], g["tails"][(0, 3)]
    assert t3[0] == (0, 12, 44, 0) and t3[1] == (1, 10, 40, 0), (t3[0], t3[1])
    assert t3[2][0] != 1 and t3[5] == T.NONE and t1[5] == T.NONE
    assert t3[3] == T.NONE and t1[3] == (0, 2, 0, 0) and t1[4][1] == 1, (t3[3], t1[3], t1[4])
    assert t3[6][0] != 4 and t3[7] == (4, 6, 8, 1), (t3[6], t3[7])
    assert t3[8] == (0, 15, 30, 0), t3[8]
    assert int(T.last_column(a, texts[8], 0)[16]) == 1 and (16 * 4) // 24 >= 1             # the one-deletion tail is a tail
    assert t3[9][:2] == (0, 20) and t3[9][3] == 1, t3[9]
    assert T.member_tail(T.last_column(d, texts[9], 0), 24, 4, 3) == (3, 0)                # the chance match is a tail of `d`
    assert t3[10][:2] == (0, 9) and t3[11][0] != 1 and t3[12] == T.NONE, (t3[10], t3[11], t3[12])
    return g


def whole_bound_group(rng):
    """k = m: every row's allowance is the row itself, so every row is a tail and the key alone decides"""
    c = b"TGGAATTCTCGGGTGCCAAGGAAC"
    panel = [c, b"ACGTTGCAACGTTGCAACGTTGCA"]
    bounds = [24, 30]
    texts = [b"TT", b"G", c[:2], rand_seq(rng, 20), rand_seq(rng, 30) + c[:10], b"CC" + c[:1]]
    g = group("whole_bound", panel, bounds, texts)
    t3 = g["tails"][(0, 3)]
    assert all(t[0] >= 0 for t in g["tails"][(0, 1)]) and all(t[0] >= 0 for t in t3)
    assert t3[0][1] >= 3 > len(texts[0]) and t3[0][3] >= t3[0][1] - 2 and t3[0][2] == 0, t3[0]      # rows past the text: deletions
    assert t3[1][3] >= 2 and t3[4][1] - t3[4][3] >= 10, (t3[1], t3[4])
    return g


def tall_group(rng):
    # (member 0: nothing past its first 40 bases matches a text of C and T, so row 128 never comes near its bound + 63)
    panel = [rand_seq(rng, 40) + rand_seq(rng, 216, "AG"), rand_seq(rng, 256), rand_seq(rng, 200), rand_seq(rng, 129)]
    bounds = [10, 60, 50, 20]
    texts = [
        rand_seq(rng, 150, "CT") + panel[0][:40],            # block 0 only: the member's bound keeps blocks 1 .. 3 out
        rand_seq(rng, 150, "CT") + panel[0][:26],
        rand_seq(rng, 30) + panel[1][:100],                  # a tail in block 1
        rand_seq(rng, 10) + mutate(rng, panel[1][:180], 20),      # ... in block 2, with errors
        rand_seq(rng, 5) + mutate(rng, panel[1][:250], 30),       # ... in block 3
        rand_seq(rng, 40) + mutate(rng, panel[2][:150], 12),
        rand_seq(rng, 64) + panel[1][:128],
        rand_seq(rng, 64) + panel[1][:192],
        rand_seq(rng, 100) + panel[3][:128],                 # the last row that can be a tail, on block 1's last row
    ]
    g = group("tall", panel, bounds, texts)
    t3 = g["tails"][(0, 3)]
    assert t3[0] == (0, 40, 150, 0) and t3[2][:2] == (1, 100) and t3[6][:2] == (1, 128) and t3[7][:2] == (1, 192), t3
    assert 64 < t3[3][1] and t3[3][0] == 1 and t3[4][0] == 1 and t3[4][1] > 192 and t3[5][0] == 2, t3
    assert (25 * 10) // 256 == 0 and t3[1] == (0, 26, 150, 0)
    # every row from 128 on is far above the bound: blocks 1 .. 3 hold no cell <= k and are not live
    assert int(T.last_column(panel[0], texts[0], 0)[128:].min()) > 10 + 63
    return g


def iupac_group(rng):
    panel = [b"ARGYTNACGTSWKMACGTBDHVAC", b"NNNNACGTACGTACGTACGTACGT", b"ACGTRYACGTRYACGTRYACGTRY"]
    bounds = [3, 2, 4]
    texts = [
        rand_seq(rng, 30, "CT") + b"AAGCTGACGTCAGC",         # member 0 through its sets
        rand_seq(rng, 30, "CT") + b"AGGTTTACGT",
        rand_seq(rng, 30) + b"GATTACGTAC",                   # member 1's N against bases
        rand_seq(rng, 30) + b"ACGTANACGTNN",                 # N in the text: all four bases / nothing / "not ACGT"
        b"N", b"NNN", b"NNNNNNNNNNNN",
        rand_seq(rng, 30) + b"ACGTRYACGTRY",                 # the text repeats the member's letters
        rand_seq(rng, 30) + b"ACGTAYACGTGC",
        rand_seq(rng, 20) + b"ACGU" + b"ACGTRUACG",          # U
        b"",
    ]
    g = group("iupac", panel, bounds, texts)
    tl = g["tails"]
    assert any(x != y for x, y in zip(tl[(0, 3)], tl[(T.IUPAC, 3)])) and any(x != y for x, y in zip(tl[(T.IUPAC, 3)], tl[(T.IUPAC_PATTERN, 3)]))
    assert tl[(T.IUPAC, 1)][4][0] >= 0 and tl[(T.IUPAC_PATTERN, 1)][4] == T.NONE and tl[(0, 1)][4][0] >= 0      # a text N under each flag
    assert tl[(T.IUPAC, 3)][0][:2] == (0, 14), tl[(T.IUPAC, 3)][0]
    return g


def random_group(rng, name, alphabet, n_texts, K):
    panel = [rand_seq(rng, int(m), alphabet) for m in rng.integers(20, 70, K)]
    bounds = [int(b) for b in rng.integers(0, 4, K)]
    texts = []
    for i in range(n_texts):
        n = int(rng.integers(1, 151))
        if i % 2:
            p = int(rng.integers(0, K))
            m = len(panel[p])
            r = int(rng.integers(6, m))
            # a base of every letter's set, then as many edits as the row allows at the most
            clean = "".join(T.I.SETS[chr(ch)][int(rng.integers(0, len(T.I.SETS[chr(ch)])))] for ch in panel[p][:r]).encode()
            tail = mutate(rng, clean, int(rng.integers(0, (r * min(bounds[p], m)) // m + 1)))
            texts.append(fit(rng, tail, max(n, 8)))
        else:
            texts.append(rand_seq(rng, n))
    return group(name, panel, bounds, texts)


def have_share(groups, key):
    tails = [t for g in groups for t in g["tails"][key]]
    return sum(t[0] >= 0 for t in tails) / len(tails)


def build():
    rng = np.random.default_rng(20261020)
    named = [lengths_group(rng), adapters_group(rng), whole_bound_group(rng), tall_group(rng), iupac_group(rng)]
    rnd = [random_group(rng, "acgt", "ACGT", 120, 6), random_group(rng, "letters", "ACGTACGTACGTACGTRYN", 60, 4)]
    for f in FLAGS:
        share = have_share(rnd, (f, 3))
        print("flag", f, "share of texts with a tail", round(share, 3))
        assert 1 / 3 <= share <= 2 / 3, (f, share)
    return {"named": named, "random": rnd}


def dump(sets):
    out = {}
    for name, groups in sets.items():
        out[name] = [{"name": g["name"], "panel": [p.decode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.decode() for t in g["texts"]],
                      "tails": {"%d:%d" % k: [list(t) for t in v] for k, v in g["tails"].items()}} for g in groups]
    with open(PATH, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


def load():
    with open(PATH) as f:
        raw = json.load(f)
    sets = {}
    for name, groups in raw.items():
        sets[name] = [{"name": g["name"], "panel": [p.encode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.encode() for t in g["texts"]],
                       "tails": {tuple(int(x) for x in k.split(":")): [tuple(t) for t in v] for k, v in g["tails"].items()}} for g in groups]
    return sets


if __name__ == "__main__":
    dump(build())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
