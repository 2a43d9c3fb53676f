"""Queued panel runs (quicked_batch_configure_panel_queue) through the library's HOST layer, built with g++ against the fake HIP
runtime under ASan + UBSan (tests/native/panel_queue_host.cpp lists what it checks): the interface's rules, the getters between
queue and fetch, and the fetched results against the definitions (tests/panel_queue_lib.py) on small groups of the recorded
sets -- the heads' and tails' named groups, whose heads or tails are the record's and whose other definitions are computed by
the same modules."""
import os
import shutil
import subprocess

import pytest

import panel_queue_lib as Q
from native_build import ASAN_UBSAN, build_host


def small_groups():
    heads = {g["name"]: g for g in Q.groups("panel_heads", "named")}
    tails = {g["name"]: g for g in Q.groups("panel_tails", "named")}
    letters = [g for g in Q.groups("panel_heads", "random") if g["name"] == "letters"]
    return [heads["adapters"], heads["edges"], tails["iupac"], tails["whole_bound"], heads["tall"]] + letters


def test_host_layer_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the host layer")
    gs = small_groups()
    assert any(b"" in g["texts"] for g in gs)
    Q.cases_file(str(tmp_path / "cases"), gs)
    exe = build_host("panel_queue_host.cpp", tmp_path, ASAN_UBSAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", QE_STUB_HBM_BYTES=str(8 << 30))
    for name in ("QE_PANEL_SLICES", "QE_PANEL_HITS_RAW_KB", "QE_PANEL_ALIGN_WS_KB", "QE_SEARCH_FORM", "QE_STUB_BOUND", "QE_STUB_SKIP_EVERY"):
        env.pop(name, None)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "panel_queue_host ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
