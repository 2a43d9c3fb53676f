"""The fixed cases of the panel-search tests (tests/test_search_panel_cpu.py, tests/test_host_search_panel.py,
tests/test_gpu_search_panel.py) and the recorder of the brute force's answers to them.

Everything is regenerated from a seed.  Two sets, each {texts, panel, bounds (one per member, cycled over 0, 1, d - 1, d,
d + 1, m, INT32_MAX with d = the member's INFIX distance to the first text it was planted in), uniform (one bound for
max_dist_all)}:

  named   member lengths 1, 24, 63, 64, 65, 128, 129, 192, 193, 256 mixed in one panel, a duplicate member at a higher index,
          two members that differ in one base, a member with R / Y / N; text lengths 1, 63, 64, 65, 127, 128, 129, 300, texts
          shorter than members, empty texts, a text holding two different members, a text holding none, texts with N
  random  200 texts x 12 members, planted as in the named set.  A plain 10 %-error set has almost no ties and few runner-ups,
          so they are constructed: texts with two members planted, near-duplicate and duplicate members in the panel.  The
          generator asserts -- by the brute force alone, INFIX, unflagged, under the uniform bound -- at least 50 texts with a
          runner-up, at least 10 with a tied best score and at least 10 with no member within its bound.

Recorded in tests/golden/search_panel_cases.json next to the sequences: per set, mode (PREFIX, INFIX) and flag (0, 16, 32) the
brute force's unbounded matrix {d, text_end} (tests/panel_lib.py).  The tests recompute a sample of it live and derive every
expectation from it through panel_lib; nothing here comes from the library.

    python tests/golden/make_search_panel_cases.py
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

import panel_lib as P      # noqa: E402

FIXTURE = os.path.join(HERE, "search_panel_cases.json")
SEED = 20261019
ACGT = b"ACGT"
MODES = (P.PREFIX, P.INFIX)
FLAGS = (0, P.IUPAC, P.IUPAC_PATTERN)
INT32_MAX = 2**31 - 1


def rand(rng, n):
    return bytes(ACGT[int(x)] for x in rng.integers(0, 4, n))


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
    """per member: 0, 1, d - 1, d, d + 1, m, INT32_MAX in turn; d = its INFIX distance to the first text it was planted in"""
    out = []
    for p, q in enumerate(panel):
        d = P.pair_answer(q, texts[planted_in[p]], P.INFIX, 0)[0] if p in planted_in else len(q) // 4
        out.append([0, 1, max(0, d - 1), d, d + 1, len(q), INT32_MAX][p % 7])
    return out


def named_set():
    rng = np.random.default_rng(SEED)
    lens = [24, 1, 63, 64, 65, 128, 129, 192, 193, 256]
    panel = [rand(rng, m) for m in lens]
    panel[1] = b"G"
    panel.append(panel[0])                                         # 10: a duplicate of member 0
    near = bytearray(panel[0]); near[11] = ACGT[(ACGT.index(near[11]) + 1) % 4]
    panel.append(bytes(near))                                      # 11: member 0 with one base changed
    base = rand(rng, 24)
    deg = bytearray(base)
    for i, code in ((2, b"R"), (7, b"Y"), (12, b"N"), (18, b"R"), (21, b"Y")):
        deg[i] = code[0]
        base = base[:i] + (b"A" if code == b"R" else (b"C" if code == b"Y" else b"G")) + base[i + 1:]
    panel.append(bytes(deg))                                       # 12: a member with R / Y / N ...
    panel.append(panel[4])                                         # 13: a duplicate of the 65-base member
    panel.append(rand(rng, 24))                                    # 14: another 24-mer
    texts, planted_in = [], {}

    def add(t, members=()):
        for p in members:
            planted_in.setdefault(p, len(texts))
        texts.append(t)

    for p in range(len(panel)):                                    # every member once, at about 8 % error, in a 300-base text
        q = base if p == 12 else panel[p]
        add(plant(rng, 300, [mutate(rng, q, 0.08)]), [p])
    for n in (1, 63, 64, 65, 127, 128, 129, 300):                  # the text lengths, each holding what fits
        fit = [p for p in (0, 2, 3, 4, 5, 6) if len(panel[p]) <= n]
        add(plant(rng, n, [mutate(rng, panel[fit[-1]], 0.05)]) [:n] if fit else rand(rng, n), fit[-1:] if fit else [])
    add(panel[5][:30])                                             # texts shorter than members
    add(mutate(rng, panel[9][100:180], 0.05))
    add(panel[7][:191])
    add(b"")                                                       # empty texts
    add(plant(rng, 150, [panel[0], panel[14]]), [0, 14])           # two different members
    add(plant(rng, 300, [mutate(rng, panel[3], 0.06), mutate(rng, panel[14], 0.1)]))
    add(b"")
    add(rand(rng, 200))                                            # none
    add(with_n(rng, plant(rng, 120, [panel[0]]), 6))               # texts with N
    add(with_n(rng, plant(rng, 200, [base]), 10))
    add(plant(rng, 90, [base[:12] + b"N" + base[13:]]))            # ... and N where the member has N
    add(panel[11] + panel[0])                                      # the near-duplicates side by side, exact
    add(panel[9])                                                  # a whole member: an exact occurrence at the text's end
    add(rand(rng, 64) + panel[4] + rand(rng, 63))
    return {"texts": texts, "panel": panel, "bounds": cycle_bounds(panel, texts, planted_in), "uniform": 6}


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
        n = int(rng.integers(40, 161))
        if kind < 11:                                              # one member at about 8 % error
            p = int(rng.integers(0, len(panel)))
            t = plant(rng, max(n, len(panel[p]) + 10), [mutate(rng, panel[p], 0.08)])
            planted_in.setdefault(p, i)
        elif kind < 16:                                            # two members
            a, b = (int(x) for x in rng.choice(8, 2, replace=False))
            t = plant(rng, 160, [mutate(rng, panel[a], 0.04), mutate(rng, panel[b], 0.04)])
        elif kind < 19:                                            # none: too short for anything within the bound
            t = rand(rng, int(rng.integers(1, 16)))
        else:
            t = with_n(rng, plant(rng, n, [panel[10]]), 4)
        texts.append(t)
    panel[10] = degenerate
    out = {"texts": texts, "panel": panel, "bounds": cycle_bounds(panel, texts, planted_in), "uniform": 3}
    hits, _, _ = P.expected(texts, panel, [out["uniform"]] * len(panel), P.INFIX, 0)
    runner = int((hits[:, 4] >= 0).sum())
    tied = int(((hits[:, 4] >= 0) & (hits[:, 5] == hits[:, 1])).sum())
    none = int(sum(1 for i, t in enumerate(texts) if t and hits[i, 0] < 0))
    assert runner >= 50 and tied >= 10 and none >= 10, (runner, tied, none)
    out["census"] = {"runner_up": runner, "tied_best": tied, "none_within_bound": none}
    return out


def record(s):
    rec = {}
    for mode in MODES:
        for flag in FLAGS:
            D, E = P.matrix(s["texts"], s["panel"], mode, flag)
            rec["%d_%d" % (mode, flag)] = {"d": D.tolist(), "end": E.tolist()}
    return rec


def load():
    """-> {"named": set, "random": set}: sequences as bytes, the recorded matrices as arrays under "matrix"[(mode, flag)]"""
    with open(FIXTURE) as f:
        raw = json.load(f)
    out = {}
    for name in ("named", "random"):
        s = raw[name]
        out[name] = {"texts": [t.encode() for t in s["texts"]], "panel": [q.encode() for q in s["panel"]], "bounds": s["bounds"],
                     "uniform": s["uniform"],
                     "matrix": {(int(k.split("_")[0]), int(k.split("_")[1])): (np.array(v["d"], dtype=np.int64), np.array(v["end"], dtype=np.int64))
                                for k, v in s["matrix"].items()}}
    return out


def main():
    doc = {"seed": SEED}
    for name, make in (("named", named_set), ("random", random_set)):
        s = make()
        rec = record(s)
        doc[name] = {"texts": [t.decode() for t in s["texts"]], "panel": [q.decode() for q in s["panel"]], "bounds": s["bounds"],
                     "uniform": s["uniform"], "matrix": rec}
        if "census" in s:
            doc[name]["census"] = s["census"]
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
