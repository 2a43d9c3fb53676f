"""Panel search, every occurrence (quicked_batch_run_panel_all): the definition, from the per-pair brute forces.

Per (text, member): search_hits_lib.occurrences (the library's equality) or iupac_lib.occurrences (the two flags) gives the
occurrences of that pattern in that text within the member's bound (clamped to m there): the valley rule, plateaus, text_start by
the best search's rule, 0 for PREFIX.  A text's occurrences are those lists concatenated in the order of the members -- each is
ordered by text_end already --, so they are ordered by (pattern, text_end).  found is their number, the stored ones are the first
max_hits, the text's score the smallest score among all found (-1: none).  An empty text has nothing.  It shares no code with
quicked_amd/csrc/qe_panel.h or qe_search.h.
"""
import iupac_lib as I
import search_hits_lib as H

PREFIX, INFIX = H.PREFIX, H.INFIX
IUPAC, IUPAC_PATTERN = I.IUPAC, I.IUPAC_PATTERN
INT32_MAX = 2**31 - 1
OCC_FIELDS = ("pattern", "text_start", "text_end", "score")


def occurrences(pattern, text, mode, flag, bound):
    """-> [(text_start, text_end, score)] of one member in one text, ordered by text_end"""
    if flag:
        return I.occurrences(bytes(pattern), bytes(text), mode, flag, bound)
    return H.occurrences(bytes(pattern), bytes(text), mode, bound)


def text_hits(text, panel, bounds, mode, flag):
    """-> [(pattern, text_start, text_end, score)] of every member in one text, ordered by (pattern, text_end), uncapped"""
    out = []
    if not text:
        return out
    for p, q in enumerate(panel):
        out += [(p, s, e, v) for s, e, v in occurrences(q, text, mode, flag, bounds[p])]
    assert out == sorted(out, key=lambda o: (o[0], o[2]))
    return out


def all_hits(texts, panel, bounds, mode, flag):
    return [text_hits(t, panel, bounds, mode, flag) for t in texts]


def capped(hits, max_hits):
    """one text's uncapped list -> (found, the stored ones, score)"""
    return len(hits), hits[:max_hits], (min(o[3] for o in hits) if hits else -1)


def best_two(hits):
    """consequence 1: -> (pattern, score, text_start, text_end, second_pattern, second_score) as a panel run reports them"""
    if not hits:
        return (-1,) * 6
    key = min((o[3], o[0]) for o in hits)
    first = next(o for o in hits if (o[3], o[0]) == key)
    others = [(o[3], o[0]) for o in hits if o[0] != key[1]]
    second = min(others) if others else (-1, -1)
    return (key[1], key[0], first[1], first[2], second[1], second[0])


def member_best(hits, k):
    """consequence 2: -> (score [k], text_end [k]): every member's smallest score and the first end that has it, -1 / -1: none"""
    sc, en = [-1] * k, [-1] * k
    for p, _, e, v in hits:
        if sc[p] < 0 or v < sc[p]:
            sc[p], en[p] = v, e
    return sc, en


def cases_file(path, s, modes, flags):
    """the input of the native programs (tests/native/panel_hits_cpu.cpp, panel_hits_host.cpp): the set -- K n nconf, K x {member
    bound}, n x text ("." = empty) -- and per (mode, flag, the members' own bounds / the uniform one) "mode flag uniform" (-1: the
    own bounds) and n x {found, found x {pattern text_start text_end score}}, uncapped, as this module defines them"""
    texts, panel = s["texts"], s["panel"]
    lines = ["%d %d %d" % (len(panel), len(texts), len(modes) * len(flags) * 2)]
    lines += ["%s %d" % (q.decode(), b) for q, b in zip(panel, s["bounds"])]
    lines += [t.decode() or "." for t in texts]
    for mode in modes:
        for flag in flags:
            for uniform in (-1, s["uniform"]):
                lines.append("%d %d %d" % (mode, flag, uniform))
                for hits in s["hits"][(mode, flag, "own" if uniform < 0 else "uniform")]:
                    lines.append(" ".join([str(len(hits))] + [str(int(v)) for o in hits for v in o]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
