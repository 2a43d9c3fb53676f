"""Bounded edit distance (quicked_batch_run_bounded), the part that needs no GPU: the public surface, and the diagonal-word
recurrence of quicked_amd/csrc/qe_bounded.h -- the source k_bounded_diag runs per lane -- compiled with g++ and driven
pair by pair against edlib (recorded in tests/golden/bounded_cases.json; live where oracle/_ref is built)."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")


def _cases():
    spec = importlib.util.spec_from_file_location("make_bounded_cases", os.path.join(ROOT, "tests", "golden", "make_bounded_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _cases()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_header_declares_the_call():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        text = f.read()
    assert re.search(r"quicked_status_t\s+quicked_batch_run_bounded\s*\(\s*quicked_batch_t\s*\*\s*batch\s*,\s*const\s+int32_t\s*\*", text)
    assert "[3] diagonal-word launches of bounded" in text


def test_exports_and_prototypes():
    from quicked_amd import capi
    assert "quicked_batch_run_bounded" in capi.EXPORTS
    lib = capi.lib()
    assert hasattr(lib, "quicked_batch_run_bounded")
    assert hasattr(capi.ResidentBatch, "run_bounded")


def test_null_batch_and_negative_bound_are_refused():
    from quicked_amd import capi
    lib = capi.lib()
    assert lib.quicked_batch_run_bounded(None, None, 8, 1, 1) == capi.QUICKED_ERROR
    assert lib.quicked_batch_run_bounded(None, None, -1, 1, 1) == capi.QUICKED_ERROR
    bounds = np.array([3, -2], dtype=np.int32)
    assert lib.quicked_batch_run_bounded(None, bounds.ctypes.data, 0, 1, 0) == capi.QUICKED_ERROR


def test_switch_is_in_the_table():
    with open(os.path.join(CSRC, "qe_pool.h")) as f:
        assert '"QE_BOUNDED_DIAG"' in f.read()


# ---- the recurrence on the CPU --------------------------------------------------------------------------------------
def _build(tmp, flags, tag):
    so = os.path.join(tmp, f"libbounded_diag_{tag}.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
           "-I" + CSRC] + flags + [os.path.join(NATIVE, "bounded_diag_cpu.cpp"), "-o", so]
    subprocess.run(cmd, check=True)
    return so


def _load(so):
    lib = C.CDLL(so)
    lib.bd_takes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.bd_distance.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int]
    lib.bd_distance_batch.argtypes = [C.c_int] + [C.c_void_p] * 8
    lib.bd_distance_batch.restype = None
    return lib


@pytest.fixture(scope="module")
def diag(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the recurrence for the host")
    return _load(_build(str(tmp_path_factory.mktemp("bounded")), [], "plain"))


def _entries(lib, pairs, dist, bounds):
    """every (pair, bound) the precondition admits, laid out as bd_distance_batch takes them, and the expected answers"""
    ent = [(i, k) for i, (p, t) in enumerate(pairs) for k in bounds if lib.bd_takes(k, len(p), len(t))]
    arr = {"plen": np.array([len(pairs[i][0]) for i, _ in ent], dtype=np.int32),
           "tlen": np.array([len(pairs[i][1]) for i, _ in ent], dtype=np.int32),
           "poff": np.zeros(len(ent), dtype=np.int64), "toff": np.zeros(len(ent), dtype=np.int64),
           "bound": np.array([k for _, k in ent], dtype=np.int32)}
    starts, pp, tp, top_p, top_t = {}, [], [], 0, 0
    for e, (i, _) in enumerate(ent):
        if i not in starts:
            starts[i] = (top_p, top_t)
            pp.append(pairs[i][0]); tp.append(pairs[i][1])
            top_p += len(pairs[i][0]); top_t += len(pairs[i][1])
        arr["poff"][e], arr["toff"][e] = starts[i]
    arr["ppool"], arr["tpool"] = b"".join(pp), b"".join(tp)
    exp = np.array([M.threshold(dist[i], k) for i, k in ent], dtype=np.int32)
    return ent, arr, exp


def _mismatches(ent, out, exp):
    return [(ent[e], int(out[e]), int(exp[e])) for e in np.nonzero(out != exp)[0][:10]]


def _sweep(lib, pairs, dist, bounds):
    """-> (entries, expected, mismatches); one native call"""
    ent, a, exp = _entries(lib, pairs, dist, bounds)
    out = np.full(len(ent), -7, dtype=np.int32)
    lib.bd_distance_batch(len(ent), a["ppool"], a["poff"].ctypes.data, a["plen"].ctypes.data, a["tpool"], a["toff"].ctypes.data,
                          a["tlen"].ctypes.data, a["bound"].ctypes.data, out.ctypes.data)
    return ent, exp, _mismatches(ent, out, exp)


def test_grid_every_bound_against_edlib(diag):
    pairs = M.grid_pairs()
    dist = M.expected("grid", pairs)
    assert diag.bd_max_bound() == M.MAX_DIAG
    ent, exp, bad = _sweep(diag, pairs, dist, range(M.MAX_DIAG + 1))
    print(f"{len(ent)} (pair, bound) entries, {int((exp >= 0).sum())} within")
    # (the precondition admits a pair only from bound |m - n| up, so most admitted entries are within their bound; both
    # answers must still be well represented -- counted on edlib's distances, before the recurrence's are looked at)
    assert len(ent) > 15000 and (exp >= 0).sum() * 8 >= len(ent) and (exp < 0).sum() * 8 >= len(ent)
    assert not bad, bad
    # every (m, n) of the grid that some bound admits was there, at every bound from |m - n| (or 0) up
    seen = {(len(pairs[i][0]), len(pairs[i][1])) for i, _ in ent}
    assert seen >= {(m, n) for m in M.LENS for n in M.LENS if abs(m - n) <= M.MAX_DIAG}
    # bounds above the limit are taken where the pair is shorter than them: the effective bound is max(m, n)
    ent2, exp2, bad2 = _sweep(diag, pairs, dist, (64, 65, 100, 1000, 2**31 - 1))
    assert ent2 and all(max(len(pairs[i][0]), len(pairs[i][1])) <= M.MAX_DIAG for i, _ in ent2)
    assert not bad2, bad2


def test_long_pairs_against_edlib(diag):
    pairs = M.long_pairs()
    dist = M.expected("long", pairs)
    ent, exp, bad = _sweep(diag, pairs, dist, (0, 1, 48, 63))
    assert len(ent) == 4 * len(pairs) - sum(1 for (p, t) in pairs for k in (0, 1, 48, 63) if abs(len(p) - len(t)) > k)
    assert (exp >= 0).any() and (exp < 0).any()
    assert not bad, bad


def test_symbol_rule_of_the_recurrence(diag):
    # case folded, every non-ACGT byte one symbol (dna_text.c:41-46)
    assert diag.bd_distance(b"ACGTN", 5, b"acgtR", 5, 5) == 0
    assert diag.bd_distance(b"ACGTN", 5, b"ACGTA", 5, 5) == 1
    assert diag.bd_distance(b"A", 1, b"C", 1, 0) == -1
    assert diag.bd_distance(b"A" * 70, 70, b"A", 1, 1000) == -2          # |m - n| = 69: not the kernel's


def test_under_address_and_undefined_sanitizers(diag, tmp_path):
    exe = str(tmp_path / "bounded_diag_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-DBD_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    os.path.join(NATIVE, "bounded_diag_cpu.cpp"), "-o", exe], check=True)
    for k, (name, pairs, bounds) in enumerate((("grid", M.grid_pairs(), (0, 1, 7, 31, 32, 62, 63, 64, 1000)),
                                               ("long", M.long_pairs(), (0, 1, 48, 63)))):
        ent, a, exp = _entries(diag, pairs, M.expected(name, pairs), bounds)
        d = tmp_path / f"set{k}"
        d.mkdir()
        for key, ext in (("plen", "i32"), ("tlen", "i32"), ("bound", "i32"), ("poff", "i64"), ("toff", "i64")):
            a[key].tofile(str(d / f"{key}.{ext}"))
        (d / "ppool.bin").write_bytes(a["ppool"]); (d / "tpool.bin").write_bytes(a["tpool"])
        r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and "bounded_diag ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        out = np.fromfile(str(d / "out.i32"), dtype=np.int32)
        assert len(out) == len(ent) and not _mismatches(ent, out, exp)
