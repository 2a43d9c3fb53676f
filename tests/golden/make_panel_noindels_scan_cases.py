"""Writes tests/golden/panel_noindels_scan_cases.json: a boundary set for the windowed mismatch-only panel run
(quicked_batch_run_panel_scan_no_indels) at windows of 64 and 128 columns, with the answers of the definition
(tests/panel_noindels_lib.py: text_hits, plain loops over bytes, no window anywhere).  Run it from the repository root:

    python tests/golden/make_panel_noindels_scan_cases.py

A list of groups {name, panel, bounds, texts, results}; results holds per flag (0, IUPAC 16, IUPAC_PATTERN 32) and text the
UNCAPPED list of INFIX occurrences [pattern, text_start, text_end, score]; steps holds per flag the group's block steps at
forced windows of 64, 128, 192 and 4096 columns by tests/panel_noindels_scan_lib.py's rule.  A group's entries are its (text,
member, flag) combinations.

copies       members of 1, 5, 24, 63, 64, 65, 100, 128, 129, 200 and 256 bases (all three block forms; members longer than the
             window), each planted with 0 or 1 substitutions so that it ends at c - 1 .. c + 2 for the first three c of 64, 128,
             192, 256, 320 that have room for it
staircases   homopolymer members A^m, bound 2, against A-texts with two planted non-A bases: R steps 2 -> 1 -> 0 with the first
             fall at c - 1 or c and the second at c + 1, c + 2 or c + 40; c the first two multiples of 128 and the first odd
             multiple of 64 that have room.  Half of the texts end 10 bases behind the second fall (the plateau of zeros reaches
             the text's end), half run on over the next multiple of 128
plateaus     A^m against A-texts with one non-A base: plateaus that rise after a boundary, fall after it, or reach the text's
             end behind it; poly-A at bounds 0 and 2
short        texts with n < m, n = m and n around 64 and 128; windows that lie wholly below m (members of 129 bases at window 64)
bounds       a clamped bound (9 on 5 bases: everything is within it) and INT32_MAX against random texts: more than 64
             occurrences in one text
bytes        R / Y / N members, a poly-N text, lower case, under all three flags

Asserted here, with the truth recorded from panel_noindels_lib.text_hits:
  (a) tests/panel_noindels_scan_lib.py's windowed model equals it on every entry at both windows;
  (b) the wrong model that takes prev = k + 1 at every c0 differs from it on at least a quarter of the (entry, window) combinations;
  (c) the wrong model that treats c1 as the text's end -- no run-out -- differs on at least a quarter.
(b) and (c) are conditions on the set: it can tell a wrong window rule from a right one.

Beside it tests/golden/panel_noindels_scan_steps.json: for every group of tests/golden/panel_noindels_cases.json (the unwindowed
run's fixture) and every flag, the block steps of its INFIX cases at forced windows of 64, 128, 192 and 4096 by the same rule --
recorded because the plain loops take a minute over the long members of that set.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import panel_noindels_lib as N  # noqa: E402
import panel_noindels_scan_lib as S  # noqa: E402

PATH = os.path.join(HERE, "panel_noindels_scan_cases.json")
STEPS_PATH = os.path.join(HERE, "panel_noindels_scan_steps.json")
WINDOWS = (64, 128)
LENS = (1, 5, 24, 63, 64, 65, 100, 128, 129, 200, 256)
MAX = N.INT32_MAX
ALL_FLAGS = (0, N.IUPAC, N.IUPAC_PATTERN)


def rand_seq(rng, n, alphabet="ACGT"):
    return bytes(ord(alphabet[int(x)]) for x in rng.integers(0, len(alphabet), n))


def substitute(rng, seq, count):
    s = bytearray(seq)
    for at in rng.choice(len(s), size=min(count, len(s)), replace=False):
        s[at] = ord("ACGT"[("ACGT".index(chr(s[at]).upper()) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(s)


def group(name, panel, bounds, texts, flags=(0,)):
    g = {"name": name, "panel": [bytes(p) for p in panel], "bounds": [int(b) for b in bounds], "texts": [bytes(t) for t in texts]}
    g["results"] = {f: [N.text_hits(t, g["panel"], g["bounds"], N.INFIX, f) for t in g["texts"]] for f in flags}
    g["steps"] = {f: S.block_steps_at(g["texts"], g["panel"], g["bounds"], f, S.NATIVE_WINDOWS) for f in flags}
    return g


def copies_groups(rng):
    out = []
    for i, m in enumerate(LENS):
        q = rand_seq(rng, m)
        bound = (0, 1, 2, MAX, 1)[i % 5] if m > 1 else 0
        texts = []
        for c in [c for c in (64, 128, 192, 256, 320) if c - 1 >= m][:3]:
            for d in (-1, 0, 1, 2):
                end = c + d
                texts.append(rand_seq(rng, end - m) + substitute(rng, q, int(rng.integers(0, 2)) if bound else 0) + rand_seq(rng, 7))
        g = group("copies%d" % m, [q], [bound], texts)
        ends = {o[2] for occ in g["results"][0] for o in occ}
        assert any(e % 64 == 0 for e in ends) and any(e % 64 == 1 for e in ends), (m, sorted(ends))
        out.append(g)
    return out


def with_bases(n, at, base=b"C"):
    t = bytearray(b"A" * n)
    for x in at:
        t[x] = base[0]
    return bytes(t)


def staircase_groups():
    out = []
    for m in LENS[1:]:
        texts = []
        both = [c for c in range(128, 2000, 128) if c - 1 >= m + 1][:2]
        odd = [c for c in range(64, 2000, 128) if c - 1 >= m + 1][:1]
        for c in both + odd:
            for j, (e1, e2) in enumerate((a, b) for a in (c - 1, c) for b in (c + 1, c + 2, c + 40)):
                if e2 - e1 > m - 1:
                    continue                                   # the two bases never share a window of the member
                n = e2 + 10 if j % 2 == 0 else (e2 // 128 + 1) * 128 + 9
                t = with_bases(n, (e1 - m - 1, e2 - m - 1))
                R = N.R_of(b"A" * m, t, N.INFIX, 0)
                assert (R[e1 - 1], R[e1], R[e2 - 1], R[e2]) == (2, 1, 1, 0), (m, c, e1, e2)
                texts.append(t)
        out.append(group("staircase%d" % m, [b"A" * m], [2], texts))
    return out


def plateau_groups():
    out = []
    for m in (5, 24, 64, 65, 100):
        texts = []
        for c in (128, 192):
            texts.append(with_bases(c + 22, (c + 1,)))                       # the plateau of zeros rises at c + 2
            texts.append(with_bases(c + 30, (c - m,)))                       # a plateau of ones that falls at c + 1
            texts.append(with_bases(c + 30, (c - m + 1,), b"g"))             # ... at c + 2
            texts.append(b"A" * (c + 5))                                     # reaches the text's end behind the boundary
            texts.append(with_bases(c + 5, (3,)))
        out.append(group("plateau%d" % m, [b"A" * m], [1], texts))
    out.append(group("polyA", [b"A" * 24, b"A" * 24, b"A" * 70], [0, 2, 2], [b"A" * 200, b"A" * 130, b"A" * 64, with_bases(200, (100, 150))]))
    return out


def short_groups(rng):
    out = []
    for m in (24, 64, 65, 129):
        q = rand_seq(rng, m)
        texts = [b""]
        for n in (m - 1, m, m + 1, 63, 64, 65, 127, 128, 129, 130, 200):
            texts.append(rand_seq(rng, n - m) + substitute(rng, q, 1) if n >= m else rand_seq(rng, n))
        out.append(group("short%d" % m, [q], [1], texts))
    return out


def bounds_group(rng):
    panel = [rand_seq(rng, 5), rand_seq(rng, 24), rand_seq(rng, 70)]
    texts = [rand_seq(rng, n) for n in (400, 130, 64, 257)]
    g = group("bounds", panel, [9, MAX, MAX], texts)
    assert sum(1 for o in g["results"][0][0] if o[0] == 0) > 64
    return g


def bytes_group():
    panel = [b"RYNACGRY", b"NNNN", b"acgtRYacgt", b"ACGTNNGG"]
    unit = b"ttGCTACGATccAGAACGATacgtagacgtACGTCTACGTNNGGacgaACGTNCGG"
    texts = [unit * 3, b"N" * 140, (unit[::-1] * 3)[:129], b"ACGTXACGTACGTZ" * 10]
    g = group("bytes", panel, [1, 1, 2, 1], texts, ALL_FLAGS)
    assert g["results"][N.IUPAC][1] and not [o for o in g["results"][N.IUPAC_PATTERN][1] if o[0] == 1]
    return g


def build():
    rng = np.random.default_rng(20261022)
    groups = copies_groups(rng) + staircase_groups() + plateau_groups() + short_groups(rng) + [bounds_group(rng), bytes_group()]
    entries = same = b = c = 0
    for g in groups:
        for flag, lists in g["results"].items():
            for t, truth in zip(g["texts"], lists):
                for p in range(len(g["panel"])):
                    entries += 1
                    want = [o for o in truth if o[0] == p]
                    for window in WINDOWS:
                        one = ([g["panel"][p]], [g["bounds"][p]])
                        got = [(p,) + o[1:] for o in S.text_hits(t, one[0], one[1], flag, window)]
                        assert got == want, (g["name"], flag, p, window, got, want)
                        same += 1
                        b += [(p,) + o[1:] for o in S.text_hits(t, one[0], one[1], flag, window, "prev")] != want
                        c += [(p,) + o[1:] for o in S.text_hits(t, one[0], one[1], flag, window, "runout")] != want
    print("entries", entries, "combinations", same, "(a)", same, "(b)", b, "(c)", c)
    assert 4 * b >= same and 4 * c >= same, (same, b, c)
    assert {len(q) for g in groups for q in g["panel"]} >= set(LENS)
    return groups


def dump(groups):
    out = [{"name": g["name"], "panel": [p.decode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.decode() for t in g["texts"]],
            "results": {str(k): v for k, v in g["results"].items()}, "steps": {str(k): v for k, v in g["steps"].items()}} for g in groups]
    with open(PATH, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


def load():
    with open(PATH) as f:
        raw = json.load(f)
    return [{"name": g["name"], "panel": [p.encode() for p in g["panel"]], "bounds": g["bounds"], "texts": [t.encode() for t in g["texts"]],
             "results": {int(k): [[tuple(o) for o in h] for h in v] for k, v in g["results"].items()},
             "steps": {int(k): v for k, v in g["steps"].items()}} for g in raw]


def unwindowed_steps():
    """{group: {flag: [steps at S.NATIVE_WINDOWS]}} over the unwindowed run's fixture"""
    with open(os.path.join(HERE, "panel_noindels_cases.json")) as f:
        raw = json.load(f)
    return {g["name"]: {str(flag): S.block_steps_at([t.encode() for t in g["texts"]], [q.encode() for q in g["panel"]], g["bounds"], flag, S.NATIVE_WINDOWS)
                        for flag in ALL_FLAGS} for g in raw}


def load_unwindowed_steps():
    with open(STEPS_PATH) as f:
        return {name: {int(k): v for k, v in per.items()} for name, per in json.load(f).items()}


if __name__ == "__main__":
    dump(build())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
    with open(STEPS_PATH, "w") as f:
        json.dump(unwindowed_steps(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", STEPS_PATH, os.path.getsize(STEPS_PATH), "bytes")
