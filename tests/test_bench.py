"""bench.py's own contract: a plain run prints the metric's line and nothing measured beside it; --dump-outputs writes what the timed path returned in its
last step, identical from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_samples_rows_beyond_the_limit(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    grf = rng.normal(size=(1000, 12)); iters = rng.integers(25, 4000, 1000).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "all"), {"grf": grf, "iters": iters})
    assert np.array_equal(np.load(tmp_path / "all" / "grf.npy"), grf)
    got = np.load(tmp_path / "all" / "iters.npy")
    assert got.dtype == np.float64 and np.array_equal(got, iters)
    assert not (tmp_path / "all" / "sample_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200 * (13 * 8 + 8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"grf": grf, "iters": iters})
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    assert len(rows) == 200 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))   # a fixed sample
    assert np.array_equal(np.load(tmp_path / "a" / "grf.npy"), grf[rows]) and np.array_equal(np.load(tmp_path / "a" / "iters.npy"), iters[rows])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 200 * (13 * 8 + 8) + 3 * 256


@pytest.mark.gpu
def test_plain_run_prints_the_metric_and_dumps_the_last_step(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    o = lines[0]
    assert o["unit"] == "solves/s" and o["higher_is_better"] is True and o["dtype"] == "f64" and o["steps"] == 5 and o["value"] > 0
    assert abs(o["value"] - 4096 * 1e3 / o["ms_per_step"]) < 1e-6 * o["value"]
    assert o["config"]["solved_frac"] == 1.0 and o["config"]["batch_per_gpu"] == 4096
    assert not {"roofline", "cpu_baseline", "latency", "summary"} & set(o)   # measured with --full only
    for name in ("grf", "iters", "status"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and len(a) == 4096 and np.array_equal(a, b), name
    assert np.load(tmp_path / "a" / "grf.npy").shape == (4096, 12) and (np.load(tmp_path / "a" / "status.npy") == 1).all()
