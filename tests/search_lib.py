"""Approximate pattern search (quicked_batch_run_search): the definition as a brute-force DP, and edlib's HW / SHW modes.

The DP is include/quicked_batch.h's text, cell for cell: D over the library's equality (case folded, every non-ACGT byte
one symbol), a top row of zeros (INFIX) or D[0][j] = j (PREFIX), d = min over e in 1 .. n of D[m][e], text_end the smallest
such e, text_start the smallest s < text_end whose stretch text[s:text_end] has global distance d to the pattern (PREFIX: 0).
It shares no code with quicked_amd/csrc/qe_search.h.  edlib (oracle/_ref/libedlib_ref.so, where it is built) is the second,
independent opinion on upper-case ACGT input; its loader here is this module's own.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDLIB_SO = os.path.join(ROOT, "oracle", "_ref", "libedlib_ref.so")
PREFIX, INFIX = 1, 2
EDLIB_MODE = {PREFIX: 1, INFIX: 2}              # EDLIB_MODE_SHW, EDLIB_MODE_HW
EDLIB_TASK_LOC = 1

_CODE = np.full(256, 4, dtype=np.int8)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k
    _CODE[_c + 32] = _k


def codes(s):
    return _CODE[np.frombuffer(bytes(s), dtype=np.uint8)]


def last_row(pattern, text, prefix):
    """D[m][0 .. n] of pattern (rows) against text (columns); top row j (prefix) or 0"""
    pc, tc = codes(pattern), codes(text)
    m, n = len(pc), len(tc)
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    out = np.empty(n + 1, dtype=np.int64)
    out[0] = m
    new = np.empty(m + 1, dtype=np.int64)
    for j in range(1, n + 1):
        new[0] = j if prefix else 0
        np.minimum(col[1:] + 1, col[:-1] + (pc != tc[j - 1]), out=new[1:])
        col = np.minimum.accumulate(new - idx) + idx          # the vertical step: min over i' <= i of new[i'] + (i - i')
        out[j] = col[m]
    return out


def locate(pattern, text, mode):
    """-> (d, text_start, text_end) without a bound"""
    row = last_row(pattern, text, mode == PREFIX)[1:]
    d = int(row.min())
    end = int(np.argmax(row == d)) + 1
    if mode == PREFIX:
        return d, 0, end
    back = last_row(pattern[::-1], text[:end][::-1], True)[1:]      # back[e - 1] = the global distance to text[end - e:end]
    assert int(back.min()) == d
    return d, end - (int(np.nonzero(back == d)[0][-1]) + 1), end


def bounded(answer, m, bound):
    """what a run with this bound reports for a pair whose unbounded answer is `answer`"""
    return answer if answer[0] <= min(bound, m) else (-1, -1, -1)


# ---- edlib ------------------------------------------------------------------------------------------------------------
class EdlibAlignConfig(C.Structure):
    _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int), ("additionalEqualities", C.c_void_p),
                ("additionalEqualitiesLength", C.c_int)]


class EdlibAlignResult(C.Structure):
    _fields_ = [("status", C.c_int), ("editDistance", C.c_int), ("endLocations", C.POINTER(C.c_int)),
                ("startLocations", C.POINTER(C.c_int)), ("numLocations", C.c_int), ("alignment", C.POINTER(C.c_ubyte)),
                ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]


_edlib = None


def have_edlib():
    return os.path.exists(EDLIB_SO)


def edlib_locate(pattern, text, mode):
    """-> [d, startLocations[0], endLocations[0] + 1] with EDLIB_TASK_LOC, no bound (end location -1 comes back as 0)"""
    global _edlib
    if _edlib is None:
        lib = C.CDLL(EDLIB_SO)
        lib.edlibAlign.restype = EdlibAlignResult
        lib.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, EdlibAlignConfig]
        lib.edlibFreeAlignResult.argtypes = [EdlibAlignResult]
        lib.edlibFreeAlignResult.restype = None
        _edlib = lib
    r = _edlib.edlibAlign(bytes(pattern), len(pattern), bytes(text), len(text), EdlibAlignConfig(-1, EDLIB_MODE[mode], EDLIB_TASK_LOC, None, 0))
    assert r.status == 0 and r.numLocations >= 1
    out = [int(r.editDistance), int(r.startLocations[0]), int(r.endLocations[0]) + 1]
    _edlib.edlibFreeAlignResult(r)
    return out
