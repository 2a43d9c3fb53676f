"""bench.py's command line and its --dump-outputs writer, on the CPU (no device run: tests/test_gpu_parity.py runs both)."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out.stdout, opt


def _outputs(n, seed=3):
    rng = np.random.default_rng(seed)
    cigars = [None if i % 17 == 5 else "".join(f"{rng.integers(1, 99)}{'MXID'[rng.integers(4)]}" for _ in range(rng.integers(1, 30)))
              for i in range(n)]
    pool, off = bytearray(), np.full(n, -1, np.int64)
    for i in rng.permutation(n):                         # strings in any order in the pool
        if cigars[i] is not None:
            off[i] = len(pool)
            pool += cigars[i].encode() + b"\0"
    outputs = {"scores": rng.integers(0, 5000, n).astype(np.int32), "status": np.where(np.arange(n) % 17 == 5, -2, 1).astype(np.int32),
               "cigar_pool": np.frombuffer(bytes(pool), np.uint8), "cigar_off": off}
    batch = types.SimpleNamespace(pattern_len=np.full(n, 400, np.int32), text_len=np.full(n, 410, np.int32))
    return outputs, batch, cigars


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_what_the_caller_got(tmp_path):
    bench = _bench()
    # the 64 MB bound: float64 scores + statuses of DUMP_MAX_PAIRS pairs, float32 CIGAR bytes, float64 sample indices / offsets
    assert 2 * 8 * bench.DUMP_MAX_PAIRS + 4 * bench.DUMP_CIGAR_BYTES + 2 * 8 * bench.DUMP_CIGAR_PAIRS + 6 * 4096 <= 64 << 20
    outputs, batch, cigars = _outputs(500)
    bench.dump_outputs(str(tmp_path / "a"), outputs, batch, seed=7)
    bench.dump_outputs(str(tmp_path / "b"), outputs, batch, seed=7)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"scores", "status", "cigar_pairs", "cigar_offsets", "cigar_bytes"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["scores"].tolist() == outputs["scores"].tolist() and a["status"].tolist() == outputs["status"].tolist()
    raw = a["cigar_bytes"].astype(np.uint8).tobytes()
    idx = a["cigar_pairs"].astype(np.int64)
    assert len(idx) == 500 and (np.diff(idx) > 0).all()
    for i, o in zip(idx, a["cigar_offsets"].astype(np.int64)):
        assert (o < 0 and cigars[i] is None) or raw[o:raw.index(b"\0", o)].decode() == cigars[i], i


def test_dump_outputs_samples_large_outputs(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_PAIRS", 64)
    monkeypatch.setattr(bench, "DUMP_CIGAR_BYTES", 20 * (2 * 810 + 1))
    outputs, batch, cigars = _outputs(300)
    bench.dump_outputs(str(tmp_path / "a"), outputs, batch, seed=7)
    bench.dump_outputs(str(tmp_path / "b"), dict(outputs, scores=outputs["scores"].copy()), batch, seed=7)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k                   # a fixed, seeded sample
    idx = a["pairs"].astype(np.int64)
    assert len(idx) == 64 and (np.diff(idx) > 0).all() and a["scores"].tolist() == outputs["scores"][idx].tolist()
    assert len(a["cigar_pairs"]) == 20
    raw = a["cigar_bytes"].astype(np.uint8).tobytes()
    for i, o in zip(a["cigar_pairs"].astype(np.int64), a["cigar_offsets"].astype(np.int64)):
        assert (o < 0 and cigars[i] is None) or raw[o:raw.index(b"\0", o)].decode() == cigars[i], i
