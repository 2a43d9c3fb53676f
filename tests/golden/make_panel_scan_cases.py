"""The window-boundary cases of the windowed panel search (quicked_batch_run_panel_scan; tests/test_panel_scan_cpu.py,
tests/test_host_panel_scan.py, tests/test_gpu_panel_scan.py) and the recorder of the brute force's answers to them.

One set, "windows", in the format of make_panel_hits_cases.py's sets, INFIX only, built around the boundaries c (multiples of 64)
of windows of 64 and 128 columns: texts of 0 .. 700 bases, members of 1 .. 256 bases -- warm-ups of 64 .. 512 columns that reach
back over several windows.  Everything is regenerated from a seed; the generator asserts, from the brute force alone
(tests/panel_hits_lib.py, tests/search_hits_lib.py), that the set holds what it is for:

  boundary ends    exact plants whose text_end is c - 1, c, c + 1, c + 2 for a boundary c, at least 8 of each
  tight warm-up    occurrences of score exactly k = the member's bound whose stretch is m + k = 64 (and 128) columns long because
                   of k inserted text bases, ending at c and at c + 1: a warm-up shorter than m + k misses them or sees them late;
                   and one of m + k = 66, ending at c + 1 and c + 2, that a warm-up of ceil(m / 64) chunks -- the bound forgotten --
                   cuts short
  plateaus         a plateau of row m that starts at or before a boundary and is decided after it, with each outcome: a later
                   rise (an occurrence), a later fall (the candidate is cancelled), the text's end several whole windows later
                   -- among them poly-A against the all-A member with bound 0 and with bound 2
  pending across c a descent in a window's last column (text_end = c), and a plateau AT the bound that is pending across c
  clamped bound    a member whose bound exceeds its length: every column is within the bound
  lengths          texts of 0, 1, 63, 64, 65, 127, 128, 129 bases
  IUPAC, caps      a member with R / Y / N, texts with N; a text with more than 64 occurrences spread over members and windows

No case is left out of any comparison, so the set's own lists have to fit the entry point's rule at the smallest window and the
largest cap: (window slots at 64) x 4096 <= 2^26.  Recorded in tests/golden/panel_scan_cases.json (a flagged list that equals the
unflagged one is stored as null); nothing here comes from the library.

    python tests/golden/make_panel_scan_cases.py
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

FIXTURE = os.path.join(HERE, "panel_scan_cases.json")
SEED = 20261021
ACGT = b"ACGT"
MODES = (PH.INFIX,)
FLAGS = (0, PH.IUPAC, PH.IUPAC_PATTERN)
CONFS = ("own", "uniform")
WINDOWS = (64, 128)


def rand(rng, n, letters=ACGT):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), n))


def bounds_of(s, conf):
    return s["bounds"] if conf == "own" else [s["uniform"]] * len(s["panel"])


def plateaus(row, k):
    """row = R[1 .. n] -> [(first column, last column, "rise" / "fall" / "end")] of every plateau of min(R, k + 1) that a descent
    to a value <= k starts (the candidates of the definition; "rise" and "end" are the occurrences)"""
    w = [min(int(v), k + 1) for v in row]
    out, n = [], len(w)
    for e in range(1, n + 1):
        if w[e - 1] >= (w[e - 2] if e > 1 else k + 1):
            continue
        j = e
        while j < n and w[j] == w[e - 1]:
            j += 1
        out.append((e, j, "end" if j == n else ("rise" if w[j] > w[e - 1] else "fall")))
    return out


def insert_bases(rng, q, k):
    """q with k bases inserted at spread-out places, each unlike both neighbours"""
    out = bytearray(q)
    for i in sorted((int((j + 1) * len(q) / (k + 1)) for j in range(k)), reverse=True):
        out[i:i] = bytes([next(c for c in ACGT if c != q[i - 1] and c != q[i])])
    return bytes(out)


def windows_set():
    rng = np.random.default_rng(SEED)
    base = rand(rng, 24)
    deg = bytearray(base)
    for i, code in ((3, b"R"), (9, b"Y"), (14, b"N"), (20, b"R")):
        deg[i] = code[0]
        base = base[:i] + (b"G" if code == b"R" else (b"T" if code == b"Y" else b"C")) + base[i + 1:]
    panel = [rand(rng, 24), rand(rng, 30), b"G", rand(rng, 61), rand(rng, 124), b"A" * 10, b"A" * 10, rand(rng, 256), bytes(deg),
             rand(rng, 200), rand(rng, 40), rand(rng, 64), rand(rng, 65), rand(rng, 62)]
    bounds = [2, 3, 5, 3, 4, 0, 2, 8, 1, 6, 1, 2, 2, 4]
    texts, marks = [], {}

    def add(t, mark=None):
        if mark:
            marks.setdefault(mark, []).append(len(texts))
        texts.append(t)

    # ---- boundary ends: exact plants of members 0 and 1 that end at c + d, nine boundaries per text, one text per d
    plants = []
    for d in (-1, 0, 1, 2):
        t = bytearray(rand(rng, 600 + int(rng.integers(0, 101))))
        for j, c in enumerate(range(64, 600, 64)):
            p = (j + d) % 2
            t[c + d - len(panel[p]):c + d] = panel[p]
            plants.append((len(texts), p, c, d))
        add(bytes(t), "boundary")
    # ---- tight warm-up: members 3 (61 + 3 = 64) and 4 (124 + 4 = 128) with k inserted bases, ending at c and at c + 1
    # ... and member 13 (62 + 4 = 66: the bound is what takes the warm-up from one chunk to two), ending at c + 1 and c + 2
    tight = []
    for p, ds in ((3, (0, 1)), (4, (0, 1)), (13, (1, 2))):
        for d in ds:
            stretch = insert_bases(rng, panel[p], bounds[p])
            assert len(stretch) == len(panel[p]) + bounds[p] and len(stretch) in (64, 128, 66)
            c = 256
            add(rand(rng, c + d - len(stretch)) + stretch + rand(rng, 150 + int(rng.integers(0, 40))), "tight")
            tight.append((len(texts) - 1, p, c + d))
    # ---- plateaus of the all-A members (5: bound 0, 6: bound 2) over boundaries
    add(rand(rng, 50, b"CT") + b"A" * 100 + rand(rng, 50, b"CT"), "rise")              # decided by a rise two boundaries later
    add(rand(rng, 30, b"CT") + b"A" * 300, "end")                                      # ... by the text's end, whole windows later
    add(b"A" * 420, "end")                                                             # poly-A from the text's first column
    add(rand(rng, 55, b"CT") + b"A" * 8 + rand(rng, 90, b"CT"), "at_bound")            # a plateau at member 6's bound across c = 64
    for c in (64, 128):                                                                # ... and one that falls after the boundary
        for attempt in range(4000):
            t = rand(rng, c - 12, b"CT") + rand(rng, 40, b"AAAAAC") + rand(rng, 30, b"CT")
            if any(a <= c < b and how == "fall" for a, b, how in plateaus(H.row_of(panel[6], t, PH.INFIX), bounds[6])):
                break
        add(t, "fall")
    # ---- lengths, each holding member 0 where it fits
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        t = bytearray(rand(rng, n))
        if n >= 24:
            t[n - 24:] = panel[0]
        add(bytes(t), "length")
    # ---- IUPAC: the degenerate member's expansion over a boundary, texts with N
    t = bytearray(rand(rng, 300)); t[128 - 10:128 + 14] = base; t[40] = t[70] = t[200] = ord("N")
    add(bytes(t), "iupac")
    t = bytearray(rand(rng, 200)); t[64 - 23:64 + 1] = base[:14] + b"N" + base[15:]
    add(bytes(t), "iupac")
    s = {"texts": texts, "panel": panel, "bounds": bounds, "uniform": 3}
    # ---- what the set is for, from the brute force
    assert max(len(t) for t in texts) <= 700 and {len(q) for q in panel} >= {1, 256}
    assert {len(texts[i]) for i in marks["length"]} == {0, 1, 63, 64, 65, 127, 128, 129}
    own = PH.all_hits(texts, panel, bounds, PH.INFIX, 0)
    census = {}
    for d in (-1, 0, 1, 2):
        census["end_c%+d" % d] = sum(1 for i, p, c, dd in plants if dd == d and any(o[0] == p and o[2] == c + d and o[3] == 0 for o in own[i]))
        assert census["end_c%+d" % d] >= 8, census
    for i, p, e in tight:
        assert (p, e - len(panel[p]) - bounds[p], e, bounds[p]) in own[i], (i, p, e, [o for o in own[i] if o[0] == p])
    census["tight"] = len(tight)

    def crossing(i, p, how, at_bound=False):
        k = min(bounds[p], len(panel[p]))
        row = H.row_of(panel[p], texts[i], PH.INFIX)
        return [(a, b) for a, b, h in plateaus(row, k) if h == how and any(a <= c < b for c in range(64, len(texts[i]), 64))
                and (not at_bound or int(row[a - 1]) == k)]

    assert crossing(marks["rise"][0], 5, "rise") and crossing(marks["rise"][0], 6, "rise")
    for i in marks["end"]:
        for p in (5, 6):                                               # poly-A against the all-A member, bound 0 and bound 2
            assert any(b - a >= 3 * 64 for a, b in crossing(i, p, "end")), (i, p)
    assert all(crossing(i, 6, "fall") for i in marks["fall"])
    assert crossing(marks["at_bound"][0], 6, "rise", at_bound=True)
    assert any(o[2] % 64 == 0 for h in own for o in h)                 # a descent in a window's last column
    assert bounds[2] > len(panel[2])                                   # the clamp to m: every column is within the bound
    assert all(int(v) <= len(panel[2]) for v in H.row_of(panel[2], texts[0], PH.INFIX))
    flagged = PH.all_hits(texts, panel, bounds, PH.INFIX, PH.IUPAC)
    for i in marks["iupac"]:
        assert any(o[0] == 8 for o in flagged[i]) and b"N" in texts[i], i
    assert set(b"RYN") <= set(panel[8])
    big = [h for h in own if len(h) > 64 and len({o[0] for o in h}) >= 3 and len({(o[2] - 1) // 64 for o in h}) >= 4]
    assert big
    census["found_over_64"] = len(big)
    assert sum((len(t) + 63) // 64 for t in texts) * 4096 <= 2**26
    s["census"] = census
    return s


def record(s):
    """per (mode, flag, conf) every text's flat list; under a flag, null where the list is the unflagged one (most texts have no N)"""
    rec = {}
    for mode in MODES:
        for conf in CONFS:
            plain = None
            for flag in FLAGS:
                hits = [[v for o in h for v in o] for h in PH.all_hits(s["texts"], s["panel"], bounds_of(s, conf), mode, flag)]
                plain = hits if flag == 0 else plain
                rec["%d_%d_%s" % (mode, flag, conf)] = hits if flag == 0 else [None if h == q else h for h, q in zip(hits, plain)]
    return rec


def load():
    """-> {"windows": set}: as make_panel_hits_cases.load() gives its sets, the lists under "hits"[(INFIX, flag, "own" / "uniform")]"""
    with open(FIXTURE) as f:
        raw = json.load(f)
    s = raw["windows"]
    hits = {}
    for k, v in s["hits"].items():
        mode, flag, conf = k.split("_")
        v = [s["hits"]["%s_0_%s" % (mode, conf)][i] if h is None else h for i, h in enumerate(v)]
        hits[(int(mode), int(flag), conf)] = [[tuple(h[i:i + 4]) for i in range(0, len(h), 4)] for h in v]
    return {"windows": {"texts": [t.encode() for t in s["texts"]], "panel": [q.encode() for q in s["panel"]], "bounds": s["bounds"],
                        "uniform": s["uniform"], "hits": hits}}


def main():
    s = windows_set()
    doc = {"seed": SEED, "windows": {"texts": [t.decode() for t in s["texts"]], "panel": [q.decode() for q in s["panel"]], "bounds": s["bounds"],
                                     "uniform": s["uniform"], "hits": record(s), "census": s["census"]}}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes", s["census"])
    assert os.path.getsize(FIXTURE) <= 1 << 20


if __name__ == "__main__":
    main()
