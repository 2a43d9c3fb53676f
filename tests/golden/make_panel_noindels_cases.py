"""Writes tests/golden/panel_noindels_cases.json: the cases of the mismatch-only panel runs (QUICKED_PANEL_NO_INDELS) with the
answers of the definition (tests/panel_noindels_lib.py: plain loops over bytes).  Run it from the repository root:

    python tests/golden/make_panel_noindels_cases.py

Two sets, "named" and "shape", each a list of groups {name, set, panel, bounds, texts, results}; results holds, per "mode:flag" (modes PREFIX 1 and INFIX 2; flags 0,
IUPAC 16, IUPAC_PATTERN 32), {"d", "e": the matrix [n][K] of {score or -1, text_end or -1}; "found": [n]; "occ": per text its
first CAP occurrences [pattern, text_start, text_end, score]}.  The best records follow from the matrix by the key order.

lengths      members of 1, 2, 24, 63, 64, 65, 128, 129, 255 and 256 bases with the bounds 0, 1, m and INT32_MAX among them; per
             member texts of n = m - 1, m, m + 1 and of 63, 64, 65 and 129 start positions, an empty text, and texts whose last
             window ends on the last bit of a 64-base plane word and one past it
homopolymer  homopolymer members against homopolymer texts: plateaus that reach the text's end, plateaus that rise before it,
             and a text with more valleys than max_hits 1 and 2
indels       five members of 24 bases, bound 1; every text holds members with exactly one deleted or one inserted base: the
             edit-distance run finds them within 1 (asserted through panel_lib), this run must not
single       a panel of one member
panel130     130 members with duplicates (the runner-up ties), so that QE_PANEL_SLICES 1 and 4096 cut it differently
wave65       65 texts of mixed lengths, the first an only text, the first 64 one wave, all of them a wave and a lane
bytes        N and lower case in both sequences; R / Y / N members and a poly-N text, for both IUPAC flags

named = lengths, homopolymer, indels, single, bytes; shape = panel130, wave65.  Every set holds texts with a member planted with
exactly one deleted or one inserted base.  Asserted for every set: in at least a third of its (text, member) entries this
definition's INFIX {score, text_end} differs from the edit-distance one of tests/panel_lib.py -- a kernel that ran the
edit-distance sweep could not pass.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import panel_lib as PL  # noqa: E402
import panel_noindels_lib as N  # noqa: E402

PATH = os.path.join(HERE, "panel_noindels_cases.json")
MODES = (N.PREFIX, N.INFIX)
FLAGS = (0, N.IUPAC, N.IUPAC_PATTERN)
CAP = 8
MAX = N.INT32_MAX


def rand_seq(rng, n, alphabet="ACGT"):
    return bytes(ord(alphabet[int(x)]) for x in rng.integers(0, len(alphabet), n))


def substitute(rng, seq, count):
    s = bytearray(seq)
    for at in rng.choice(len(s), size=min(count, len(s)), replace=False):
        s[at] = ord("ACGT"[("ACGT".index(chr(s[at]).upper()) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(s)


def plant(rng, n, piece):
    """a random text of n bases with `piece` somewhere in it (cut at the back if it does not fit)"""
    if len(piece) >= n:
        return piece[:n]
    at = int(rng.integers(0, n - len(piece) + 1))
    return rand_seq(rng, at) + piece + rand_seq(rng, n - at - len(piece))


def delete_one(seq, at):
    return seq[:at] + seq[at + 1:]


def insert_one(seq, at):
    base = b"ACGT"[(b"ACGT".index(seq[at:at + 1].upper()) + 2) % 4:][:1]
    return seq[:at] + base + seq[at:]


def group(name, panel, bounds, texts):
    g = {"name": name, "panel": [bytes(p) for p in panel], "bounds": [int(b) for b in bounds], "texts": [bytes(t) for t in texts]}
    g["results"] = N.results_of(g["texts"], g["panel"], g["bounds"], CAP)
    return g


def differing_cells(g):
    """per (text, member) entry: is the INFIX {score, text_end} not the edit-distance run's"""
    texts, panel = g["texts"], g["panel"]
    D, E = PL.cut(*PL.matrix(texts, panel, N.INFIX, 0), panel, g["bounds"])
    res = g["results"][(N.INFIX, 0)]
    return [(int(D[i][p]), int(E[i][p])) != (res["d"][i][p], res["e"][i][p]) for i in range(len(texts)) for p in range(len(panel))]


def lengths_group(rng):
    lens = [1, 2, 24, 63, 64, 65, 128, 129, 255, 256]
    panel = [rand_seq(rng, m) for m in lens]
    bounds = [1, MAX, 2, 63, 0, MAX, 1, 129, MAX, 0]                     # 0, 1, m (63, 129) and INT32_MAX among them
    texts = [b""]
    for p, m in enumerate(lens):
        for n in (m - 1, m, m + 1, m + 62, m + 63, m + 64, m + 128):
            texts.append(plant(rng, n, substitute(rng, panel[p], int(rng.integers(0, 3)))))
    # the last window ends on the last bit of a plane word, and one past it
    for p in (2, 5):
        for n in (128, 129, 192, 193):
            texts.append(rand_seq(rng, n - lens[p]) + substitute(rng, panel[p], 1))
    g = group("lengths", panel, bounds, texts)
    starts = {len(t) - m + 1 for t in texts for m in lens}
    assert starts >= {0, 1, 2, 63, 64, 65, 129}
    res = g["results"][(N.INFIX, 0)]
    for i in (len(texts) - 8, len(texts) - 7):                         # member 2 ends the text
        assert res["e"][i][2] == len(texts[i]) and res["d"][i][2] == 1, (i, res["d"][i][2], res["e"][i][2])
    return g


def homopolymer_group():
    panel = [b"AAAAA", b"A" * 64, b"A" * 70, b"CCCCC", b"AAAAA"]
    bounds = [0, 1, 2, 1, 5]
    texts = [b"A" * n for n in (4, 5, 6, 64, 70, 133)]
    texts += [b"A" * 10 + b"C" + b"A" * 10,                             # a plateau of zeros that rises, one that reaches the end
              b"A" * 10 + b"C" + b"A" * 4,                              # ... and one that never comes back down
              (b"AAAAAC") * 6,                                         # more valleys than max_hits 1 and 2
              b"C" * 7 + b"A" * 70 + b"C" * 7,
              b"A" * 64 + b"C" + b"A" * 64]
    g = group("homopolymer", panel, bounds, texts)
    res = g["results"][(N.INFIX, 0)]
    assert [o for o in res["occ"][6] if o[0] == 0] == [(0, 0, 5, 0), (0, 11, 16, 0)], res["occ"][6]
    assert res["found"][8] > 2 and sum(1 for o in N.text_hits(texts[8], panel, bounds, N.INFIX, 0) if o[0] == 0) == 6
    assert [tuple(o) for o in res["occ"][0]] == [] and res["found"][1] >= 1
    return g


def indels_group(rng):
    panel = [rand_seq(rng, 24) for _ in range(5)]
    bounds = [1] * 5
    texts = []
    for i in range(12):
        pieces = []
        for p in range(5):
            at = 3 + (i + 4 * p) % 18
            variant = (delete_one, insert_one)[(i + p) % 2](panel[p], at)
            pieces.append(rand_seq(rng, int(rng.integers(2, 9))) + variant)
        texts.append(b"".join(pieces) + rand_seq(rng, 5))
    texts.append(plant(rng, 90, panel[0]))                              # the controls: exact, and one substitution
    texts.append(plant(rng, 90, substitute(rng, panel[1], 1)))
    g = group("indels", panel, bounds, texts)
    D, _ = PL.cut(*PL.matrix(texts, panel, N.INFIX, 0), panel, bounds)
    res = g["results"][(N.INFIX, 0)]
    for i in range(12):
        for p in range(5):
            assert 0 <= D[i][p] <= 1 and res["d"][i][p] == -1, (i, p, D[i][p], res["d"][i][p])
    assert res["d"][12][0] == 0 and res["d"][13][1] == 1
    return g


def single_group(rng):
    q = rand_seq(rng, 24)
    texts = [plant(rng, 60, q), plant(rng, 60, substitute(rng, q, 2)), plant(rng, 60, substitute(rng, q, 3)), rand_seq(rng, 23), b""]
    texts += [plant(rng, 70, delete_one(q, 5 + i)) for i in range(3)] + [plant(rng, 70, insert_one(q, 7 + i)) for i in range(3)]
    return group("single", [q], [2], texts)


def panel130_group(rng):
    panel = [rand_seq(rng, int(rng.integers(16, 31))) for _ in range(130)]
    panel[7] = panel[3]
    panel[129] = panel[64]
    panel[66] = panel[64]
    bounds = [MAX if p % 2 == 0 else 2 for p in range(130)]
    bounds[3] = bounds[7] = 2
    texts = []
    for i in range(10):
        picks = [3, 64, int(rng.integers(0, 130))] if i < 4 else [int(x) for x in rng.integers(0, 130, 2)]
        texts.append(b"".join(rand_seq(rng, int(rng.integers(3, 12))) + substitute(rng, panel[p], int(rng.integers(0, 3))) for p in picks))
    texts.append(rand_seq(rng, 9) + delete_one(panel[3], 8) + rand_seq(rng, 6) + insert_one(panel[65], 11) + rand_seq(rng, 4))      # planted indels
    g = group("panel130", panel, bounds, texts)
    res = g["results"][(N.INFIX, 0)]
    tie = N.reduce_text(res["d"][0], res["e"][0], panel)
    assert tie[0] in (3, 64) and tie[4] in (7, 66) and tie[1] == tie[5], tie       # a duplicate is the runner-up at the best's score
    return g


def wave65_group(rng):
    panel = [rand_seq(rng, m) for m in (12, 20, 33, 64, 70)]
    bounds = [12, 1, MAX, 2, 0]
    texts = []
    for i in range(65):
        n = (0, 11, 40, 75, 130, 200, 64, 128)[i % 8] if i else 150
        p = i % 5
        piece = substitute(rng, panel[p], i % 3) if i % 4 else (delete_one, insert_one)[i // 4 % 2](panel[p], 6)      # every fourth: a planted indel
        texts.append(plant(rng, n, piece) if n else b"")
    return group("wave65", panel, bounds, texts)


def bytes_group(rng):
    panel = [b"ACGTNACGTacgtn", b"RYNACGRY", b"NNNN", b"acgtRYacgt", b"ACGTACGT"]
    bounds = [2, MAX, 1, 3, 1]
    texts = [b"ttACGTNACGTACGTNgg", b"acgtnacgtACGTN", b"N" * 16, b"ttGCTACGATccAGAACGAT", b"acgtagacgtACGTCTACGT", b"ACGTXACGTACGTZ",
             b"ACGNACGTNNACGAACGT", b"acgtacgaACGTACGT", b"UCGUACGUacgu"]
    g = group("bytes", panel, bounds, texts)
    r0, r1, r2 = (g["results"][(N.INFIX, f)] for f in FLAGS)
    assert r0["d"][2][2] == 0 and r1["d"][2][2] == 0 and r2["d"][2][2] == -1      # the poly-N text against NNNN under each reading
    assert r1["d"][3][1] == 0 and r0["d"][3][1] > 0                              # R / Y / N as sets and as the fifth symbol
    assert r0["d"][1][0] == 0                                                    # case is folded, N = n
    return g


def build():
    rng = np.random.default_rng(20261021)
    sets = {"named": [lengths_group(rng), homopolymer_group(), indels_group(rng), single_group(rng), bytes_group(rng)],
            "shape": [panel130_group(rng), wave65_group(rng)]}
    for name, groups in sets.items():
        cells = []
        for g in groups:
            g["set"] = name
            c = differing_cells(g)
            print(name, g["name"], "entries", len(c), "that differ from the edit-distance run", round(sum(c) / len(c), 3))
            cells += c
        assert max(b for g in groups for b in g["bounds"]) >= 1 and sum(cells) / len(cells) >= 1 / 3, (name, sum(cells) / len(cells))
    groups = sets["named"] + sets["shape"]
    assert sorted({len(g["panel"]) for g in groups}) == [1, 5, 10, 130]
    return groups


def dump(groups):
    out = [{"name": g["name"], "set": g["set"], "panel": [p.decode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.decode() for t in g["texts"]],
            "results": {"%d:%d" % k: v for k, v in g["results"].items()}} for g in groups]
    with open(PATH, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


def load():
    with open(PATH) as f:
        raw = json.load(f)
    return {g["name"]: {"name": g["name"], "set": g["set"], "panel": [p.encode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.encode() for t in g["texts"]],
                        "results": {tuple(int(x) for x in k.split(":")): {"d": v["d"], "e": v["e"], "found": v["found"], "occ": [[tuple(o) for o in h] for h in v["occ"]]}
                                    for k, v in g["results"].items()}} for g in raw}


if __name__ == "__main__":
    dump(build())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
