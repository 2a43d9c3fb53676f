"""The fixed cases of the all-occurrences panel tests (tests/test_panel_hits_cpu.py, tests/test_host_panel_hits.py,
tests/test_gpu_panel_hits.py) and the recorder of the brute force's answers to them.

Everything is regenerated from a seed.  Two sets, each {texts, panel, bounds (one per member, cycled over 0, 1, d - 1, d, d + 1,
m / 4, 2 with d = the member's INFIX distance to the first text it was planted in; a member of one base gets 0), uniform (one
bound for max_dist_all; it exceeds the shortest members' lengths, so the clamp to m is in play)}:

  named   member lengths 24, 1, 63, 64, 65, 128, 129, 192, 193, 256 in one panel, duplicate members at higher indices, two
          tandem-repeat members (poly-A, AC), a member with R / Y / N; text lengths 1, 63, 64, 65, 127, 128, 129, 200, texts
          shorter than their members, empty texts, one member twice in a text, two different members in one text, tandem
          repeats that make a plateau in row m, a plateau that reaches the end of the text, a text with no occurrence (under the
          members' own bounds).  The generator asserts each of these from the brute force.
  random  200 texts x 12 members, constructed by planting: one member, one member twice, two members, texts too short for
          anything, texts with N.  The generator asserts -- by the brute force alone, INFIX, unflagged, under the uniform bound --
          at least 30 texts with two or more occurrences of one member, at least 30 with occurrences of two or more members, at
          least 10 with none and at least 10 whose found exceeds 2 (the tests' caps are 1, 2 and 64).

Recorded in tests/golden/panel_hits_cases.json next to the sequences: per set, mode (PREFIX, INFIX), flag (0, 16, 32) and bounds
(own, uniform) every text's uncapped list of {pattern, text_start, text_end, score} (tests/panel_hits_lib.py).  The tests
recompute a sample of it live; nothing here comes from the library.

    python tests/golden/make_panel_hits_cases.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import panel_hits_lib as PH      # noqa: E402
import search_hits_lib as H      # noqa: E402

FIXTURE = os.path.join(HERE, "panel_hits_cases.json")
SEED = 20261020
ACGT = b"ACGT"
MODES = (PH.PREFIX, PH.INFIX)
FLAGS = (0, PH.IUPAC, PH.IUPAC_PATTERN)
CONFS = ("own", "uniform")


def rand(rng, n, letters=ACGT):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), n))


def mutate(rng, s, rate):
    """s with substitutions, insertions and deletions at about `rate` per base"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(ACGT[int(rng.integers(0, 4))])
        if r < rate:
            out.append(ACGT[(ACGT.index(c) + 1 + int(rng.integers(0, 3))) % 4] if c in ACGT else ACGT[0])
        else:
            out.append(c)
    return bytes(out)


def plant(rng, n, pieces):
    """a random text of about n bases that holds the pieces, in order, at random places"""
    room = max(0, n - sum(len(q) for q in pieces))
    cuts = sorted(int(x) for x in rng.integers(0, room + 1, len(pieces)))
    out, last = b"", 0
    for q, c in zip(pieces, cuts):
        out += rand(rng, c - last) + q
        last = c
    return out + rand(rng, room - last)


def with_n(rng, s, k):
    b = bytearray(s)
    for i in rng.integers(0, len(b), k):
        b[int(i)] = ord("N")
    return bytes(b)


def cycle_bounds(panel, texts, planted_in):
    out = []
    for p, q in enumerate(panel):
        d = min(v for _, _, v in H.occurrences(q, texts[planted_in[p]], PH.INFIX, len(q))) if p in planted_in else len(q) // 4
        out.append(0 if len(q) == 1 else [0, 1, max(0, d - 1), d, d + 1, len(q) // 4, 2][p % 7])
    return out


def bounds_of(s, conf):
    return s["bounds"] if conf == "own" else [s["uniform"]] * len(s["panel"])


def named_set():
    rng = np.random.default_rng(SEED)
    lens = [24, 1, 63, 64, 65, 128, 129, 192, 193, 256]
    panel = [rand(rng, m) for m in lens]
    panel[1] = b"G"
    panel.append(panel[0])                                         # 10: a duplicate of member 0
    panel.append(b"A" * 10)                                        # 11: a tandem repeat of one base
    base = rand(rng, 24)
    deg = bytearray(base)
    for i, code in ((2, b"R"), (7, b"Y"), (12, b"N"), (18, b"R"), (21, b"Y")):
        deg[i] = code[0]
        base = base[:i] + (b"A" if code == b"R" else (b"C" if code == b"Y" else b"G")) + base[i + 1:]
    panel.append(bytes(deg))                                       # 12: a member with R / Y / N
    panel.append(rand(rng, 24))                                    # 13: another 24-mer
    panel.append(panel[4])                                         # 14: a duplicate of the 65-base member
    panel.append(b"AC" * 6)                                        # 15: a tandem repeat of two bases
    texts, planted_in, marks = [], {}, {}

    def add(t, members=(), mark=None):
        for p in members:
            planted_in.setdefault(p, len(texts))
        if mark:
            marks[mark] = len(texts)
        texts.append(t)

    for p in range(len(panel)):                                    # every member once, at about 8 % error
        q = base if p == 12 else panel[p]
        add(plant(rng, 200 if len(q) < 190 else 300, [mutate(rng, q, 0.08)]), [p])
    for n in (1, 63, 64, 65, 127, 128, 129, 200):                  # the text lengths, each holding what fits
        fit = [p for p in (0, 2, 3, 4, 5, 6) if len(panel[p]) <= n]
        add(plant(rng, n, [mutate(rng, panel[fit[-1]], 0.05)])[:n] if fit else rand(rng, n), fit[-1:] if fit else [])
    add(panel[5][:30])                                             # texts shorter than their members
    add(mutate(rng, panel[9][100:180], 0.05))
    add(panel[7][:191])
    add(b"")                                                       # empty texts
    add(plant(rng, 200, [mutate(rng, panel[0], 0.05), panel[0]]), mark="twice")            # one member twice
    add(plant(rng, 200, [panel[0], panel[13]]), mark="two_members")                        # two different members
    add(b"")
    add(rand(rng, 40, b"CT") + b"A" * 16 + rand(rng, 40, b"CT"), mark="plateau")           # tandem repeats: plateaus in row m
    add(rand(rng, 30, b"GT") + b"AC" * 10 + rand(rng, 30, b"GT"))
    add(rand(rng, 50, b"CT") + b"A" * 14, mark="plateau_to_end")                           # ... one that reaches the text's end
    add(rand(rng, 100, b"CT"), mark="none")                                                # no occurrence under the own bounds
    add(with_n(rng, plant(rng, 120, [panel[0]]), 6))               # texts with N
    add(with_n(rng, plant(rng, 200, [base]), 10))
    add(plant(rng, 90, [base[:12] + b"N" + base[13:]]))            # ... and N where the member has N
    add(panel[9])                                                  # a whole member: an exact occurrence at the text's end
    add(rand(rng, 64) + panel[4] + rand(rng, 63))
    s = {"texts": texts, "panel": panel, "bounds": cycle_bounds(panel, texts, planted_in), "uniform": 6}
    # ---- what the set is for, from the brute force
    own = PH.all_hits(texts, panel, s["bounds"], PH.INFIX, 0)
    uni = PH.all_hits(texts, panel, bounds_of(s, "uniform"), PH.INFIX, 0)
    assert sum(1 for o in uni[marks["twice"]] if o[0] == 0) >= 2, uni[marks["twice"]]
    assert {0, 13} <= {o[0] for o in uni[marks["two_members"]]}
    assert texts[marks["none"]] and not own[marks["none"]], own[marks["none"]]
    for mark, member in (("plateau", 11), ("plateau_to_end", 11)):
        t = texts[marks[mark]]
        row = H.row_of(panel[member], t, PH.INFIX)
        ends = [o[2] for o in uni[marks[mark]] if o[0] == member]
        flat = [e for e in ends if e < len(t) and row[e] == row[e - 1]]
        assert flat, (mark, ends)
        if mark == "plateau_to_end":
            assert any(all(row[j] == row[e - 1] for j in range(e - 1, len(t))) for e in flat), (ends, list(row[-16:]))
    return s


def random_set():
    rng = np.random.default_rng(SEED + 1)
    panel = [rand(rng, int(m)) for m in (24, 24, 30, 30, 20, 36, 40, 28, 70, 130, 24, 32)]
    near = bytearray(panel[0]); near[7] = ACGT[(ACGT.index(near[7]) + 2) % 4]
    panel[1] = bytes(near)                                         # a near-duplicate of member 0
    panel[3] = panel[2]                                            # a duplicate of member 2
    deg = bytearray(panel[10]); deg[3] = ord("R"); deg[15] = ord("N")
    degenerate = bytes(deg)
    texts, planted_in = [], {}
    for i in range(200):
        kind = i % 20
        n = int(rng.integers(60, 161))
        if kind < 5:                                               # one member at about 8 % error
            p = int(rng.integers(0, len(panel)))
            t = plant(rng, max(n, len(panel[p]) + 10), [mutate(rng, panel[p], 0.08)])
            planted_in.setdefault(p, i)
        elif kind < 10:                                            # one member twice
            p = int(rng.integers(4, 8))
            t = plant(rng, 160, [mutate(rng, panel[p], 0.04), mutate(rng, panel[p], 0.04)])
        elif kind < 15:                                            # two members
            a, b = (int(x) for x in rng.choice(np.arange(4, 9), 2, replace=False))
            t = plant(rng, 200, [mutate(rng, panel[a], 0.04), mutate(rng, panel[b], 0.04)])
        elif kind < 18:                                            # none: too short for anything within the bound
            t = rand(rng, int(rng.integers(1, 16)))
        elif kind == 18:
            t = with_n(rng, plant(rng, n, [panel[10]]), 4)
        else:                                                      # a member three times in a row
            p = int(rng.integers(4, 8))
            t = plant(rng, 160, [panel[p] + mutate(rng, panel[p], 0.05) + panel[p]])
        texts.append(t)
    panel[10] = degenerate
    s = {"texts": texts, "panel": panel, "bounds": cycle_bounds(panel, texts, planted_in), "uniform": 3}
    uni = PH.all_hits(texts, panel, bounds_of(s, "uniform"), PH.INFIX, 0)
    twice = sum(1 for h in uni if any(sum(1 for o in h if o[0] == p) >= 2 for p in range(len(panel))))
    members = sum(1 for h in uni if len({o[0] for o in h}) >= 2)
    none = sum(1 for t, h in zip(texts, uni) if t and not h)
    over = sum(1 for h in uni if len(h) > 2)
    assert twice >= 30 and members >= 30 and none >= 10 and over >= 10, (twice, members, none, over)
    s["census"] = {"one_member_twice": twice, "two_members": members, "none": none, "found_over_2": over}
    return s


def record(s):
    rec = {}
    for mode in MODES:
        for flag in FLAGS:
            for conf in CONFS:
                hits = PH.all_hits(s["texts"], s["panel"], bounds_of(s, conf), mode, flag)
                rec["%d_%d_%s" % (mode, flag, conf)] = [[v for o in h for v in o] for h in hits]
    return rec


def load():
    """-> {"named": set, "random": set}: sequences as bytes, the recorded lists under "hits"[(mode, flag, "own" / "uniform")] as
    per text [(pattern, text_start, text_end, score)]"""
    with open(FIXTURE) as f:
        raw = json.load(f)
    out = {}
    for name in ("named", "random"):
        s = raw[name]
        hits = {}
        for k, v in s["hits"].items():
            mode, flag, conf = k.split("_")
            hits[(int(mode), int(flag), conf)] = [[tuple(h[i:i + 4]) for i in range(0, len(h), 4)] for h in v]
        out[name] = {"texts": [t.encode() for t in s["texts"]], "panel": [q.encode() for q in s["panel"]], "bounds": s["bounds"],
                     "uniform": s["uniform"], "hits": hits}
    return out


def main():
    doc = {"seed": SEED}
    for name, make in (("named", named_set), ("random", random_set)):
        s = make()
        doc[name] = {"texts": [t.decode() for t in s["texts"]], "panel": [q.decode() for q in s["panel"]], "bounds": s["bounds"],
                     "uniform": s["uniform"], "hits": record(s)}
        if "census" in s:
            doc[name]["census"] = s["census"]
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(HERE, "search_hits_cases.json"))


if __name__ == "__main__":
    main()
