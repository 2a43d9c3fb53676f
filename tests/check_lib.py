"""The CIGAR validator (quicked_batch_validate, quicked_batch_configure(check=1); quicked_amd/csrc/qe_check.h) restated in
Python, for the CPU and GPU tests, with the cases both run.  Nothing here comes from the library.

The rules.  A string is "<len><op>" repeated.  Operations are M X I D, and '=' is read as M.  A length is decimal, at least 1
and at most 2^31 - 1.  Digits without an operation, an operation without digits and any other byte give 0.  M needs equal
bytes, X different ones -- raw bytes, no case folding, no wildcard --, I consumes text, D consumes pattern; the first
operation that would leave a sequence gives 0; both sequences must be consumed exactly.  Lengths are Python integers here,
so a run of 2^31 bases costs nothing and cannot wrap."""
import re

import numpy as np

M, X, I, D = 0, 1, 2, 3
LETTER = "MXID"
MAX_LEN = 2 ** 31 - 1
_OPS = {ord("M"): M, ord("="): M, ord("X"): X, ord("I"): I, ord("D"): D}


def _raw(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def parse(string):
    """-> [(op, len)] of a string that keeps the syntax, else None.  The string ends at its first NUL, as in C."""
    runs, num, have = [], 0, False
    for c in _raw(string).split(b"\0")[0]:
        if 48 <= c <= 57:
            num, have = num * 10 + (c - 48), True
            if num > MAX_LEN:
                return None
            continue
        if c not in _OPS or not have or num == 0:
            return None
        runs.append((_OPS[c], num))
        num, have = 0, False
    return None if have else runs


def verdict_ops(pattern, text, ops):
    """the walk over [(op, len)]: 1 / 0.  An entry of length <= 0 is no operation (the segment form has them); None in the
    list is a leaf without runs (its buffer overflowed): 0"""
    m, n, v, h = len(pattern), len(text), 0, 0
    for e in ops:
        if e is None:
            return 0
        op, cnt = e
        if cnt <= 0:
            continue
        if op == I:
            if cnt > n - h:
                return 0
            h += cnt
        elif op == D:
            if cnt > m - v:
                return 0
            v += cnt
        else:
            if cnt > m - v or cnt > n - h:
                return 0
            a, b = pattern[v:v + cnt], text[h:h + cnt]
            if op == M and a != b:
                return 0
            if op != M and any(x == y for x, y in zip(a, b)):
                return 0
            v, h = v + cnt, h + cnt
    return 1 if (v == m and h == n) else 0


def verdict(pattern, text, string):
    """1 valid, 0 not, -1 no string"""
    if string is None:
        return -1
    runs = parse(string)
    return 0 if runs is None else verdict_ops(pattern, text, runs)


def oracle_can_judge(string):
    """what the oracle's expander (rle_to_ops) can parse: "<len><op>" with op in MXID -- it knows no '=' -- and every length
    at least 1 (it would expand a zero length to nothing, where the library's rule refuses it); short enough to expand"""
    s = _raw(string).decode("latin-1")
    if not re.fullmatch(r"(?:\d+[MXID])*", s):
        return False
    lens = [int(n) for n in re.findall(r"\d+", s)]
    return all(k >= 1 for k in lens) and sum(lens) < 10000


def to_string(runs):
    return "".join(f"{n}{LETTER[o]}" for o, n in runs)


# ---- pairs with an alignment known by construction --------------------------------------------------------------------
def random_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tolist()) if n else b""


def mutate_with_runs(rng, pattern, error):
    """-> (text, runs): substitutions, insertions and deletions at rate `error`; `runs` is the alignment that made the text
    (equal neighbours merged), valid by construction -- not an optimal one, which a validator does not ask for"""
    text, ops = bytearray(), []
    for b in pattern:
        r = rng.random()
        if r < error / 3:
            text.append(int(rng.choice([c for c in b"ACGT" if c != b])))
            ops.append(X)
        elif r < 2 * error / 3:
            text.append(int(rng.choice(list(b"ACGT"))))
            text.append(b)
            ops += [I, M]
        elif r < error:
            ops.append(D)
        else:
            text.append(b)
            ops.append(M)
    runs = []
    for o in ops:
        if runs and runs[-1][0] == o:
            runs[-1][1] += 1
        else:
            runs.append([o, 1])
    return bytes(text), [(o, n) for o, n in runs]


# ---- mutators of a valid string (runs in, string out; None where the string offers nothing to mutate) ------------------
def mut_last_run(runs, delta):
    return to_string(runs[:-1] + [(runs[-1][0], runs[-1][1] + delta)]) if runs else None


def mut_append(runs, tail):
    return to_string(runs) + tail


def mut_prepend(runs, head):
    return head + to_string(runs)


def mut_drop_last(runs):
    return to_string(runs[:-1]) if runs else None


def mut_i_to_d(runs):
    for k, (o, n) in enumerate(runs):
        if o == I:
            return to_string(runs[:k] + [(D, n)] + runs[k + 1:])
    return None


def mut_swap(runs, k):
    if len(runs) < 2:
        return None
    k %= len(runs) - 1
    return to_string(runs[:k] + [runs[k + 1], runs[k]] + runs[k + 2:])


# ---- the cases: (label, pattern, text, string) ------------------------------------------------------------------------
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 63, 64, 65, 130, 300)
BIG = 2147483647


def _sub(seq, j, byte=None):
    s = bytearray(seq)
    s[j] = byte if byte is not None else {65: 67, 67: 71, 71: 84, 84: 65}[s[j]]
    return bytes(s)


def _m_x_m(m, j):
    return "".join(f"{n}{o}" for n, o in ((j, "M"), (1, "X"), (m - j - 1, "M")) if n > 0)


def byte_lane_cases():
    """every byte lane of the M compare -- the 8-byte words and the scalar tail: one substituted position, everywhere"""
    rng = np.random.default_rng(5101)
    c = []
    for m in (1, 7, 8, 9, 16, 17, 23):
        p = random_seq(rng, m)
        for j in range(m):
            t = _sub(p, j)
            c.append((f"lane m={m} j={j} M", p, t, f"{m}M"))
            c.append((f"lane m={m} j={j} MXM", p, t, _m_x_m(m, j)))
    return c


def x_branch_cases():
    """X runs of 1, 2 and 9: one position with equal bytes (first, middle, last) is invalid, all different is valid; bare
    and between M runs"""
    rng = np.random.default_rng(5102)
    c = []
    for ln in (1, 2, 9):
        for pre, post in ((0, 0), (3, 4), (8, 0), (0, 9)):
            p = random_seq(rng, pre + ln + post)
            t = bytearray(p)
            for k in range(ln):
                t[pre + k] = _sub(p, pre + k)[pre + k]
            s = "".join(f"{n}{o}" for n, o in ((pre, "M"), (ln, "X"), (post, "M")) if n > 0)
            c.append((f"x len={ln} ctx={pre},{post} all different", p, bytes(t), s))
            for k in sorted({0, ln // 2, ln - 1}):
                u = bytearray(t)
                u[pre + k] = p[pre + k]
                c.append((f"x len={ln} ctx={pre},{post} equal at {k}", p, bytes(u), s))
    return c


def valid_pairs():
    """(pattern, text, runs) at 8-10 % error over the lengths, alignments known by construction"""
    rng = np.random.default_rng(5103)
    out = []
    for m in LENGTHS:
        for rep in range(2 if m < 15 else 3):
            p = random_seq(rng, m)
            t, runs = mutate_with_runs(rng, p, 0.08 + 0.01 * rep)
            out.append((p, t, runs))
    return out


def count_cases():
    """-> (valid cases, mutants): valid strings of mutated pairs and what the mutators make of them"""
    pairs = [q for q in valid_pairs() if len(q[0]) >= 15]
    good = [(f"valid m={len(p)} #{k}", p, t, to_string(r)) for k, (p, t, r) in enumerate(valid_pairs())]
    mutants = []
    for k, (p, t, r) in enumerate(pairs):
        other = pairs[(k + 1) % len(pairs)][2]
        made = [("last+1", mut_last_run(r, +1)), ("last-1", mut_last_run(r, -1)), ("drop last", mut_drop_last(r)),
                ("I->D", mut_i_to_d(r)), ("swap", mut_swap(r, 3 * k + 1)), ("swap2", mut_swap(r, 7 * k)), ("other pair's", to_string(other))]
        for unit in ("1I", "1D", "1M"):
            made += [("append " + unit, mut_append(r, unit)), ("prepend " + unit, mut_prepend(r, unit))]
        mutants += [(f"mutant m={len(p)} #{k} {name}", p, t, s) for name, s in made if s is not None]
    return good, mutants


def raw_byte_cases():
    weird = bytes([0x00, 0x80, 0xFF, 0x41, 0x00, 0x7F, 0xFF, 0x80, 0x01, 0xFE, 0x00])
    c = [("a vs A as M", b"a", b"A", "1M"), ("a vs A as X", b"a", b"A", "1X"),
         ("N vs N as M", b"N", b"N", "1M"), ("N vs N as X", b"N", b"N", "1X"),
         ("N vs A as M", b"N", b"A", "1M"), ("acgt vs ACGT as M", b"acgtacgtac", b"ACGTACGTAC", "10M"),
         ("acgt vs ACGT as X", b"acgtacgtac", b"ACGTACGTAC", "10X"),
         ("bytes 00 80 FF equal", weird, weird, f"{len(weird)}M"), ("bytes 00 80 FF equal as X", weird, weird, f"{len(weird)}X")]
    for j, b in ((0, 0x80), (1, 0x00), (2, 0x7F), (4, 0x30), (7, 0x00), (10, 0x80)):      # the sign bit, NUL against '0'
        t = _sub(weird, j, b)
        c.append((f"bytes 00 80 FF, position {j} -> {b:#x} as M", weird, t, f"{len(weird)}M"))
        c.append((f"bytes 00 80 FF, position {j} -> {b:#x} as MXM", weird, t, _m_x_m(len(weird), j)))
    return c


def syntax_cases():
    p7 = b"ACGTACG"
    c = [("empty string, empty pair", b"", b"", ""), ("empty string, non-empty pair", p7, p7, ""),
         ("empty string, text only", b"", b"AC", ""), ("2I, text only", b"", b"AC", "2I"), ("2D, pattern only", b"AC", b"", "2D"),
         ("3=2X valid", b"ACGTA", b"ACGCC", "3=2X"), ("3=2X invalid", b"ACGTA", b"ACGTC", "3=2X"), ("3=2X short pair", b"ACGT", b"ACGC", "3=2X")]
    for s in ("7M", "7", "M", "0M", "7Q", "7m", " 7M", "7M ", "-1M", "+7M", "7 M", "007M", "7=", "7M0I", "0I7M", "3M4", "3MM4M", "3M4M", "7N", "7S", "7H", "7P",
              "7M\n", "7.0M", "2147483648M", "7M2147483648I", "123456789012345678901234567890M", "7M123456789012345678901234567890I"):
        c.append((f"syntax {s!r}", p7, p7, s))
    return c


def length_cases(limit_itself):
    """the lengths at the parser's limit (limit_itself: 2^31 - 1, which it admits) or past it (which it refuses), on a pair
    the rest of the string is valid for.  Those past the limit fail the syntax whatever a walk would do with them; those at
    the limit leave the pair at once, and a walk that adds in 32 bits may go on outside it: not for a GPU"""
    p, t = b"ACGTACGTAC", b"ACGTACGTAC"
    c = []
    for big in ((BIG,) if limit_itself else (2147483648, 4294967296, 4294967297, 4294967306, 18446744073709551617, 10 ** 29 + 1)):
        for op in "MXID":
            c.append((f"length {big}{op} first", p, t, f"{big}{op}10M"))
            c.append((f"length {big}{op} last", p, t, f"10M{big}{op}"))
            c.append((f"length {big}{op} alone", p, t, f"{big}{op}"))
    return c


def wrap_cases_in_range():
    """I and D runs of 2^31 - 1 whose sums, taken modulo 2^32, are back in range before any M or X, then the pair's valid
    string.  A walk that adds lengths in 32 bits reads only inside the pair on these and accepts them; they are invalid: the
    first run already leaves the sequence"""
    c = []
    ins = (f"{BIG}I{BIG}I2I", f"{BIG}I1I{BIG}I1I")
    dels = (f"{BIG}D{BIG}D2D", f"{BIG}D1D{BIG}D1D")
    both = (f"{BIG}I{BIG}D{BIG}I{BIG}D2I2D", f"{BIG}D1D{BIG}I1I{BIG}I{BIG}D1D1I")
    for p, t, r in [q for q in valid_pairs() if len(q[0]) in (0, 9, 17, 64, 300)][::2]:
        for k, head in enumerate(ins + dels + both):
            c.append((f"wrap back into range m={len(p)} head {k}", p, t, head + to_string(r)))
    return c


def wrap_cases_out_of_range():
    """the wraps that leave a 32-bit walk OUTSIDE the pair when an M or X follows: never for a GPU, only for the sanitizer
    build of the walk on the CPU"""
    c = []
    for p, t, r in [q for q in valid_pairs() if len(q[0]) in (9, 17, 64)][::3]:
        good = to_string(r)
        m, n = len(p), len(t)
        heads = [f"{BIG}I1I", f"{BIG}D1D", f"{BIG}I1I{BIG}D1D", f"{BIG}I2I", f"{BIG}D2D",             # INT_MIN landings and next to them
                 f"{BIG}I{BIG}I1I", f"{BIG}D{BIG}D1D", f"{BIG}I{BIG}I3I", f"{BIG}D{BIG}D3D",          # -1 and +1 around the start
                 f"{BIG}D2D", f"{BIG}I{BIG}I2I{BIG}D2D"]
        for k, head in enumerate(heads):
            c.append((f"wrap out of range m={m} head {k}", p, t, head + good))
            c.append((f"wrap out of range m={m} head {k} then 1M", p, t, head + "1M" + good))
            c.append((f"wrap out of range m={m} head {k} then 9X", p, t, head + "9X" + good))
        for op in "MX":
            # v + cnt and h + cnt past 2^31 after a first step; with v or h negative the sum lands in range
            c.append((f"wrap sum m={m} 1{op}{BIG}{op}", p, t, f"1{op}{BIG}{op}"))
            c.append((f"wrap sum m={m} 1M{BIG}{op}", p, t, f"1M{BIG}{op}"))
            c.append((f"wrap sum m={m} 1I{BIG}{op}", p, t, f"1I{BIG}{op}"))
            c.append((f"wrap sum m={m} 1D{BIG}{op}", p, t, f"1D{BIG}{op}"))
            c.append((f"wrap sum m={m} {BIG}D2D{BIG}{op}", p, t, f"{BIG}D2D{BIG}{op}"))
            c.append((f"wrap sum m={m} {BIG}I2I{BIG}{op}", p, t, f"{BIG}I2I{BIG}{op}"))
            c.append((f"wrap sum m={m} {BIG}I2I{BIG}D2D{BIG}{op}", p, t, f"{BIG}I2I{BIG}D2D{BIG}{op}{good}"))
            c.append((f"wrap sum m={m} {BIG}I1I{BIG}D1D{BIG}{op}1{op}", p, t, f"{BIG}I1I{BIG}D1D{BIG}{op}1{op}{good}"))
        # undone by a later run, with the pair's own string in between
        c.append((f"wrap undone later m={m}", p, t, f"{BIG}I{good}{BIG}I2I"))
        c.append((f"wrap undone later m={m} D", p, t, f"{BIG}D{good}{BIG}D2D"))
        c.append((f"wrap to the end m={m}", p, t, f"{BIG}I{BIG}I{n + 2}I{BIG}D{BIG}D{m + 2}D"))
    return c


def long_string_cases():
    """one lane with a 200 000-character string.  "1M1I1D" repeated consumes two bases of each sequence per six characters, so
    on a 300-base pair the 200 000 characters are reached with zero-padded lengths (150 units, 450 runs); the plain form gets
    the pair it needs: 33 333 units, 66 666 bases.  The second string of each has one count off"""
    rng = np.random.default_rng(5104)

    def pair_of(units):
        p, t = bytearray(), bytearray()
        for _ in range(units):
            a, b, c2 = (int(x) for x in rng.choice(list(b"ACGT"), 3))
            p += bytes([a, c2]); t += bytes([a, b])                       # 1M: a == a; 1I: b into the text; 1D: c2 off the pattern
        return bytes(p), bytes(t)

    c = []
    p, t = pair_of(150)
    width = 200000 // 450 - 1                                              # digits per length: 450 runs of width + 1 characters

    def pad(n):
        return str(n).rjust(width, "0")

    body = (pad(1) + "M" + pad(1) + "I" + pad(1) + "D") * 150
    good = "0" * (200000 - len(body)) + body                               # what is left over: zeros in front of the first length
    assert len(good) == 200000 and len(p) == 300 and len(t) == 300
    c.append(("200 000 characters, zero-padded 1M1I1D, 300 bases", p, t, good))
    c.append(("200 000 characters, zero-padded 1M1I1D, 300 bases, last count 2", p, t, good[:-(width + 1)] + pad(2) + "D"))
    p, t = pair_of(33333)
    plain = "00" + "1M1I1D" * 33333
    assert len(plain) == 200000
    k = 6 * 20000 + 2
    c.append(("200 000 characters, 1M1I1D, 66 666 bases", p, t, plain))
    c.append(("200 000 characters, 1M1I1D, 66 666 bases, one count 2", p, t, plain[:k] + "2" + plain[k + 1:]))
    return c


_memo = {}


def gpu_cases():
    """every case a GPU may see: small pairs, and no string that could take a 32-bit walk outside its pair"""
    if "gpu" not in _memo:
        good, mutants = count_cases()
        _memo["gpu"] = (byte_lane_cases() + x_branch_cases() + good + mutants + raw_byte_cases() + syntax_cases() + length_cases(False) +
                        wrap_cases_in_range() + long_string_cases())
    return _memo["gpu"]


def cpu_cases():
    """the GPU's cases and those that must never go to a GPU untested"""
    if "cpu" not in _memo:
        _memo["cpu"] = gpu_cases() + length_cases(True) + wrap_cases_out_of_range()
    return _memo["cpu"]
