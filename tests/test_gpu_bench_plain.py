"""A plain ``bench.py --gpus 1`` run: exactly ``--steps`` timed iterations, the headline line without the ``--full``
objects, and ``--dump-outputs`` files that are the same from run to run (the inputs are seeded)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("best_cost", "best_knots", "argmin_cost", "argmin_seed", "argmin_knots")


def _run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines and p.stdout.rstrip().endswith(lines[-1]), p.stdout[-2000:]
    return json.loads(lines[-1]), {n: np.load(os.path.join(out_dir, f"{n}.npy")) for n in NAMES}


def test_plain_run_times_the_steps_and_dumps_what_they_computed(device, tmp_path):
    line, a = _run(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 7 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f32"
    rollouts = line["config"]["rollouts_per_step_per_gpu"]
    assert line["value"] == pytest.approx(rollouts / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for key in ("roofline", "cpu_baseline", "ik", "full_record"):
        assert key not in line, key  # measured only with --full
    seeds = line["config"]["seeds_per_gpu"]
    assert a["best_cost"].shape == (seeds,) and a["best_knots"].shape[0] == seeds
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.isfinite(a["best_cost"]).all() and np.isfinite(a["best_knots"]).all()
    k = int(a["argmin_seed"][0])
    assert a["argmin_cost"][0] == a["best_cost"].min() == a["best_cost"][k]
    np.testing.assert_array_equal(a["argmin_knots"][0], a["best_knots"][k])
    # same arguments, same inputs: a second process computes the same outputs
    _, b = _run(tmp_path / "b")
    for n in NAMES:
        np.testing.assert_allclose(b[n], a[n], rtol=1e-5, atol=1e-6, err_msg=n)
