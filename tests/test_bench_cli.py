"""bench.py's command line: a plain run times its steps and prints the result line, --dump-outputs
writes what the last timed step computed, and everything else waits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("cpu_baseline", "topk30", "topk30_users_per_s", "mfma_busy_profiled")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_options_default_to_a_plain_run(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_validated(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def _run(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "c2", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out), *extra], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(gpu_lib, tmp_path):
    """c2 (1M x 200K, rank 64): both sides' factors exceed the per-side cap and are written as the
    seeded row sample; two runs with the same arguments write the same arrays."""
    import bench
    line, out = _run(tmp_path, "a")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["nnz"] / (line["ms_per_step"] / 1000.0), rel=1e-9)
    assert all(line[key] is None for key in FULL_ONLY) and line["config"]["top5_degrees"] is None
    assert sorted(os.listdir(out)) == ["item_factors.npy", "user_factors.npy"]
    line_b, out_b = _run(tmp_path, "b")
    total = 0
    for name in ("user_factors", "item_factors"):
        f = np.load(out / f"{name}.npy")
        assert f.dtype == np.float32 and f.shape == (bench.DUMP_SIDE_BYTES // (4 * 64), 64)
        assert np.isfinite(f).all() and np.abs(f).max() > 0
        assert np.array_equal(f, np.load(out_b / f"{name}.npy"))
        total += f.nbytes
    assert total <= 64 * 1000 * 1000
