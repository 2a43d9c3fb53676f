"""Queued panel runs (quicked_batch_configure_panel_queue), the part that needs no GPU: the public surface, the overflow rule on the
definition, and the per-slot steps of the queued all-occurrences run -- panel_queue_expand_slot, panel_queue_finish_one and
panel_queue_clamp_one of quicked_amd/csrc/qe_panel.h, the source k_panel_queue_expand, _finish and _clamp run per thread --
compiled with g++ as a stand-alone program (tests/native/panel_queue_cpu.cpp), plain and under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import panel_queue_lib as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "quicked_amd", "csrc")


def test_header_documents_the_contract():
    with open(os.path.join(ROOT, "include", "quicked_batch.h")) as f:
        flat = " ".join(f.read().split()).replace(" * ", " ")
    assert "quicked_status_t quicked_batch_configure_panel_queue(quicked_batch_t* batch, int64_t max_total);" in flat
    assert "int64_t quicked_batch_panel_queue_wanted(quicked_batch_t* batch);" in flat
    for phrase in ("0, the default of every batch, is off", "1 .. 2^26 is on", "leaves the setting unchanged",
                   "Runs with sync != 0 never look at the setting", "The panel and max_dist are read during the call",
                   "every getter answers exactly as before the call", "everything the sync run leaves, bit for bit",
                   "hit_off'[i] = min(hit_off[i], max_total)", "stored'[i] = hit_off'[i + 1] - hit_off'[i]",
                   "the first max_total of the sync run's array", "counter [0] counts the block steps really walked",
                   "a cap per text shows as stored < found, a cap per run as wanted > total",
                   "returns W after such a fetch, and -1 after anything else",
                   "QUICKED_PANEL_MATRIX; QUICKED_PANEL_CIGARS (the host reads the strings' total); quicked_batch_run_panel_scan; quicked_batch_run_search_all",
                   "Not built: queued runs with the matrix or the strings"):
        assert phrase in flat, phrase


def test_exports_and_signatures_without_a_device():
    from quicked_amd import capi
    assert {"quicked_batch_configure_panel_queue", "quicked_batch_panel_queue_wanted"} <= set(capi.EXPORTS)
    assert callable(capi.ResidentBatch.configure_panel_queue) and callable(capi.ResidentBatch.panel_queue_wanted)
    lib = capi.lib()
    assert lib.quicked_batch_configure_panel_queue.argtypes == [C.c_void_p, C.c_int64] and lib.quicked_batch_configure_panel_queue.restype == C.c_int
    assert lib.quicked_batch_panel_queue_wanted.argtypes == [C.c_void_p] and lib.quicked_batch_panel_queue_wanted.restype == C.c_int64
    assert lib.quicked_batch_configure_panel_queue(None, 16) == capi.QUICKED_ERROR
    assert lib.quicked_batch_panel_queue_wanted(None) == -1


def test_the_overflow_rule_by_hand():
    lists = [[(0, 0, 4, 0), (1, 2, 9, 1), (1, 5, 12, 0)], [], [(2, 1, 3, 2)], [(0, 0, 1, 0), (0, 3, 4, 1)]]
    found, off, recs, scores, W = Q.capped_run(lists, 2, 1 << 20)
    assert (found, off, W, scores) == ([3, 0, 1, 2], [0, 2, 2, 3, 5], 5, [0, -1, 2, 0]) and len(recs) == 5
    _, off3, recs3, scores3, W3 = Q.capped_run(lists, 2, 3)                # on a text's boundary
    assert off3 == [0, 2, 2, 3, 3] and recs3 == recs[:3] and W3 == 5 and scores3 == scores
    assert Q.capped_run(lists, 2, 1)[1] == [0, 1, 1, 1, 1] and Q.capped_run(lists, 2, 4)[1] == [0, 2, 2, 3, 4]      # inside a stretch
    assert Q.capped_run(lists, 2, 5)[1:3] == Q.capped_run(lists, 2, 6)[1:3] == (off, recs)


def test_the_groups_hold_what_the_tests_need():
    """every fixture's named and random sets load, with empty texts among them, and the definitions a fixture does not record
    come out of the same functions as those it does (a sample of the tails' set against its record)"""
    seen = 0
    for fixture in Q.FIXTURES:
        for name in ("named", "random"):
            gs = Q.groups(fixture, name)
            assert gs, (fixture, name)
            seen += sum(len(g["texts"]) for g in gs)
    assert seen > 1500 and any(b"" in g["texts"] for g in Q.groups("panel_hits", "named"))
    g = Q.groups("panel_tails", "named")[1]
    assert Q.tails(g, 0, 3) == g["tails"][(0, 3)]
    import panel_tails_lib as T
    assert T.all_tails(g["texts"], g["panel"], g["bounds"], 16, 3) == g["tails"][(16, 3)]
    assert any(h for h in Q.hits(g, Q.INFIX, 0)) and len(Q.heads(g, 0, 3)) == len(g["texts"])


def _build(tmp, flags, tag):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the steps for the host")
    exe = os.path.join(tmp, f"panel_queue_cpu_{tag}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags +
                   [os.path.join(NATIVE, "panel_queue_cpu.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("tag, flags", [("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_capped_expand_finish_and_clamp_equal_the_restatement(tmp_path, tag, flags):
    exe = _build(str(tmp_path), flags, tag)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"panel_queue_cpu ok layouts (\d+) records (\d+) without_occurrence (\d+)", r.stdout)
    assert m and int(m.group(1)) > 300 and int(m.group(2)) > 100000 and int(m.group(3)) > 0, r.stdout
