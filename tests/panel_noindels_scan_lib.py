"""The windowed mismatch-only panel run (quicked_batch_run_panel_scan_no_indels): the window rule, by plain
loops over panel_noindels_lib.R_of.

A text of n bases is cut into window slots (c0, c1], c0 = 0, window, 2 window .. and c1 = min(c0 + window, n).  Per member of m
bases and effective bound k a slot reads w[e] = min(R[e], k + 1) and does three things:

  prev at c0    c0 >= m: w[c0], the value of start c0 - m, which the slot computes but does not own.  c0 < m: k + 1, "higher
                than every value"; the first owned end is then m.  c1 < m: the slot owns nothing and walks nothing.
  owned ends    (c0, c1], from max(c0 + 1, m): a descent of w makes a candidate, a rise emits the pending one.
  run-out       the ends past c1, one by one and only while a candidate is pending: a rise or the text's end emits it, a descent
                clears it (that valley's first end is a later slot's).

The block steps a slot walks per member: the starts from max(0, c0 - m) up to the last one it computed -- c1 - m, or further
by the run-out -- times ceil(m / 64).

`wrong` names two deliberately wrong rules, for the fixture's conditions: "prev" takes k + 1 at every c0, "runout" treats c1 as
the text's end.
"""
import panel_noindels_lib as N

INFIX = N.INFIX


def slots(n, window):
    """-> [(c0, c1)] of a text of n bases; window 0: one slot"""
    if n <= 0:
        return []
    if window <= 0:
        return [(0, n)]
    return [(c0, min(c0 + window, n)) for c0 in range(0, n, window)]


def slot_walk(R, m, k, n, c0, c1, wrong=None):
    """one member against one slot -> ([(text_end, score)] the slot owns, the starts it walked)"""
    if c1 < m:
        return [], 0
    high = k + 1

    def w(e):
        return min(R[e], high)

    prev = w(c0) if c0 >= m and wrong != "prev" else high
    first_start = max(0, c0 - m)
    out, pend = [], None
    e = max(c0 + 1, m)
    while e <= c1:                                  # the owned ends
        v = w(e)
        if v < prev:
            pend = (e, v)
        elif v > prev and pend is not None:
            out.append(pend)
            pend = None
        prev = v
        e += 1
    if wrong == "runout" and pend is not None:
        out.append(pend)
        pend = None
    while pend is not None and e <= n:              # the run-out
        v = w(e)
        if v < prev:
            pend = None
        elif v > prev:
            out.append(pend)
            pend = None
        prev = v
        e += 1
    if pend is not None:                            # the text's end
        out.append(pend)
    return out, e - m - first_start


def text_walk(text, panel, bounds, flag, window, wrong=None):
    """-> ([(pattern, text_start, text_end, score)] in (pattern, text_end) order, uncapped; the block steps of the text's slots)"""
    hits, steps = [], 0
    n = len(text)
    for p, q in enumerate(panel):
        m, k = len(q), N.bound_of(bounds, p, q)
        R = N.R_of(q, text, INFIX, flag)
        for c0, c1 in slots(n, window):
            got, walked = slot_walk(R, m, k, n, c0, c1, wrong)
            hits += [(p, e - m, e, v) for e, v in got]
            steps += walked * ((m + 63) // 64)
    return hits, steps


def block_steps_at(texts, panel, bounds, flag, windows):
    """block_steps for several forced windows at once -> [steps per window] (R is computed once per text and member)"""
    out = [0] * len(windows)
    for text in texts:
        n = len(text)
        for p, q in enumerate(panel):
            m, k = len(q), N.bound_of(bounds, p, q)
            R = N.R_of(q, text, INFIX, flag)
            for i, window in enumerate(windows):
                out[i] += sum(slot_walk(R, m, k, n, c0, c1)[1] for c0, c1 in slots(n, window)) * ((m + 63) // 64)
    return out


def text_hits(text, panel, bounds, flag, window, wrong=None):
    return text_walk(text, panel, bounds, flag, window, wrong)[0]


def block_steps(texts, panel, bounds, flag, window):
    """counter [0] of a run at a forced window (> 0)"""
    return sum(text_walk(t, panel, bounds, flag, window)[1] for t in texts)


NATIVE_WINDOWS = (64, 128, 192, 4096)


def cases_file(path, groups):
    """the input of the native programs (tests/native/panel_noindels_scan_cpu.cpp, panel_noindels_scan_host.cpp): "ngroups", then
    per group "K n nconf", K x {member bound}, n x text ("." = empty) and per flag "flag" with the group's block steps at the
    windows of NATIVE_WINDOWS (a group's "steps", where it has them recorded per flag, else computed here), and n x {found,
    found x {pattern text_start text_end score}}: the uncapped lists of panel_noindels_lib.text_hits"""
    lines = ["%d" % len(groups)]
    for g in groups:
        flags = sorted(g["results"])
        lines.append("%d %d %d" % (len(g["panel"]), len(g["texts"]), len(flags)))
        lines += ["%s %d" % (q.decode(), b) for q, b in zip(g["panel"], g["bounds"])]
        lines += [t.decode() or "." for t in g["texts"]]
        for flag in flags:
            steps = g["steps"][flag] if flag in g.get("steps", {}) else block_steps_at(g["texts"], g["panel"], g["bounds"], flag, NATIVE_WINDOWS)
            lines.append(" ".join(str(v) for v in [flag] + list(steps)))
            for occ in g["results"][flag]:
                lines.append(" ".join(str(int(v)) for v in [len(occ)] + [x for o in occ for x in o]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
