"""bench.py's result line and --dump-outputs: a plain run reports the headline figure alone, and the outputs it dumps are
what the timed path handed its caller in the last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kkt_prim", "kkt_dual", "cpu_baseline", "other_configs", "extra_fp32_inner_preconditioner")


def _bench(args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path):
    """above the size limit every array is cut to the same seeded sample of its rows, written with the row numbers beside it"""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import bench; bench.DUMP_LIMIT = 1 << 16; "
            "x = np.arange(6000, dtype=np.float64).reshape(1000, 6); "
            "bench.dump_outputs(sys.argv[1], dict(x=x, y=np.arange(3000, dtype=np.float32)))" % ROOT)
    for d in ("a", "b"):
        subprocess.run([sys.executable, "-c", code, str(tmp_path / d)], check=True, timeout=120)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["x.npy", "x_rows.npy", "y.npy", "y_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= (1 << 16) + 4 * 128       # + the .npy headers
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    x, rows = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "x_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(x, np.arange(6000, dtype=np.float64).reshape(1000, 6)[rows])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path, gpu_required):
    """C1 through the single-QP path: --steps sets the timed steps, no --full extras, x and y of the last solve in float64"""
    from qpdo_amd import problems, solver
    d = _bench(["--workload", "C1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY), sorted(d)
    assert d["steps"] == 3 and len(d["status_val"]) == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert sorted(os.listdir(tmp_path)) == ["x.npy", "y.npy"]
    x, y = np.load(tmp_path / "x.npy"), np.load(tmp_path / "y.npy")
    assert x.dtype == y.dtype == np.float64
    r = solver.solve_problem(problems.config_qp("C1"), verbose=0)
    assert r["info"]["status_val"] == 1 and x.shape == r["x"].shape and y.shape == r["y"].shape
    assert np.abs(x - r["x"]).max() <= 1e-9 * max(1.0, np.abs(r["x"]).max())
    assert np.abs(y - r["y"]).max() <= 1e-9 * max(1.0, np.abs(r["y"]).max())


@pytest.mark.gpu
def test_plain_batch_run_dumps_every_item_of_the_last_step(tmp_path, gpu_required):
    """C3 through the batch stream: x and y of every item of the last step, item by item as solve_batch returns them"""
    from qpdo_amd import problems, solver
    count = 64
    d = _bench(["--workload", "C3", "--steps", "3", "--warmup", "1", "--batch-count", str(count), "--max-iter", "300",
                "--dump-outputs", str(tmp_path)])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY), sorted(d)
    assert d["steps"] == 3 and d["items"] == 3 * count
    x, y = np.load(tmp_path / "x.npy"), np.load(tmp_path / "y.npy")
    cfg = problems.CONFIGS["C3"]
    assert x.dtype == y.dtype == np.float64 and x.shape == (count, cfg["n"]) and y.shape == (count, cfg["m"])
    res, failed = solver.solve_batch([problems.config_qp("C3", i) for i in range(count)], verbose=0, max_iter=300)
    assert failed == 0
    for i, r in enumerate(res):
        assert np.abs(x[i] - r["x"]).max() <= 1e-12 * max(1.0, np.abs(r["x"]).max()), i
        assert np.abs(y[i] - r["y"]).max() <= 1e-12 * max(1.0, np.abs(r["y"]).max()), i
