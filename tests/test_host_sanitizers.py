"""The HOST layer of libquicked_hip.so under sanitizers, without a GPU (the reference offers ASAN / UBSAN for its whole
library, CMakeLists.txt:43-49).  quicked_amd/csrc/qe_driver.hip (host half), qe_stages.hip, qe_pool.h, qe_batch.h, qe_capi.cpp and
qe_hostpack.cpp are built with g++ against tests/native/hip_stub -- a header-compatible fake of the HIP runtime calls they
use, device memory = host memory under a byte budget, kernels = host stand-ins run at launch -- and driven through the C-ABI
by tests/native/host_scenarios.cpp: rotation of queued runs and fetches, early finish and merged flows, thread churn on
leased contexts, per-pair calls from several threads, reclaim under a device-memory budget."""
import os
import shutil
import subprocess

import pytest

from native_build import ASAN_UBSAN, build_host


def run(exe, env_extra, timeout=600):
    env = dict(os.environ, QE_FINISHERS="3", **env_extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout, env=env)
    return r


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_layer_under_thread_sanitizer(tmp_path):
    exe = build_host("host_scenarios.cpp", tmp_path, ["-fsanitize=thread"])
    env = {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1", "QE_STUB_HBM_BYTES": str(8 << 30)}
    r = run(exe, env)
    assert r.returncode == 0 and "host_scenarios ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    # A race shows up under load, not alone: round 5's lease race (qe::ctx() reset a context's fields before it held the
    # context's `busy` mutex while a reclaiming thread could still be writing them) was silent in 15 of 15 lone runs and
    # reported in 7 of 30 when six copies of the binary shared the machine.  So: rounds of six copies side by side, >= 50
    # runs in all, none of which may report anything (QE_TSAN_ROUNDS: more rounds for a soak, 0 to skip).
    rounds = int(os.environ.get("QE_TSAN_ROUNDS", "9"))
    full = dict(os.environ, QE_FINISHERS="3", **env)
    for rnd in range(rounds):
        procs = [subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=full) for _ in range(6)]
        for k, p in enumerate(procs):
            try:
                out, err = p.communicate(timeout=600)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise AssertionError(f"round {rnd}, copy {k}: the host scenarios did not finish (a deadlock?)")
            assert p.returncode == 0 and "host_scenarios ok" in out, (rnd, k, (out + err)[-6000:])
            assert "WARNING: ThreadSanitizer" not in err, (rnd, k, err[-6000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_layer_under_address_and_ub_sanitizers(tmp_path):
    exe = build_host("host_scenarios.cpp", tmp_path, ASAN_UBSAN)
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "QE_STUB_HBM_BYTES": str(8 << 30)})
    assert r.returncode == 0 and "host_scenarios ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    # a device too small for two threads' pools: the staged out-of-memory path (qe_pool.h) must carry both through
    r = subprocess.run([exe, "budget"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", QE_STUB_HBM_BYTES=str(700 << 20), QE_OOM_WAIT_MS="2000",
                                QE_STUB_EXPECT_RECLAIM="1"))
    assert r.returncode == 0 and "host_scenarios ok" in r.stdout, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
