"""The span classifier of k_pack (quicked_amd/csrc/qe_pack.h), the part that needs no GPU: tests/native/pack_cpu.cpp packs
sequences span by span as the kernel's lanes do -- the header's own source, with v_perm_b32 as a byte loop -- and compares planes, padding rows and flags with a byte-at-a-time scalar packer written from
the reference's code table: the lengths across every boundary of the scheme, ACGT in both cases, N / n, the IUPAC letters,
bytes 0x00 0x7F 0x80 0xFF, random bytes, all 256 byte values at every position of a lane, forward and reversed.  The same
program runs plain and under ASan + UBSan; it is a stand-alone program, nothing is loaded into Python.  The numpy rule of
tests/pack_lib.py, which the GPU test compares with, is held to the same scalar packer's answers on a few strings here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pack_lib as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the classifier for the host")
    exe = os.path.join(tmp, f"pack_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "pack_cpu.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "pack ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_lane_walk_equals_the_scalar_packer(tmp_path):
    out = _run(_build(str(tmp_path), [], "plain"))
    assert int(out.split()[2]) >= 2 * (6 * 22 * 2 + 2 * 2 * 16 * 256)


def test_under_address_and_undefined_sanitizers(tmp_path):
    _run(_build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "asan"))


def test_header_is_what_the_kernel_runs():
    with open(os.path.join(CSRC, "qe_kernels.hip")) as f:
        src = f.read()
    assert '#include "qe_pack.h"' in src
    body = src[src.index("void pack_span("):src.index("void k_pack(PackArgs A)")]
    assert "pack_classify16(" in body and "pack_flags16(" in body and "pack_fetch16(" in body


def test_numpy_rule_on_known_strings():
    w, f = P.ref_pack(b"ACGTNa")
    assert [int(x) for x in w] == [0x6, 0xC, 0x10, 0, 0, 0, 0, 0, 0] and f == P.FLAG_HAS_N | P.FLAG_NONCANON
    w, f = P.ref_pack(b"ACGTNa", reverse=True)
    assert [int(x) for x in w[:3]] == [0b011000, 0b001100, 0b000010] and f == 3
    w, f = P.ref_pack(b"G" * 64 + b"T")
    assert [int(x) for x in w[:6]] == [2**64 - 1, 2**64 - 1, 0, 0, 1, 0] and f == 0 and len(w) == 3 * 4
    assert P.ref_pack(b"")[0].tolist() == [0] * 6 and P.ref_pack(b"N")[1] == P.FLAG_HAS_N and P.ref_pack(b"n")[1] == 3
    assert P.ref_pack(bytes([0x80]))[1] == 3 and P.ref_pack(b"t")[1] == P.FLAG_NONCANON
    words, off, flags = P.ref_pack_set([b"A" * 65, b"", b"C"])
    assert off.tolist() == [0, 12, 18] and len(words) == 27 and flags.tolist() == [0, 0, 0] and words.dtype == np.uint64
