"""``bench.py --gpus N`` plumbing on the test box's ONE GPU (gloo ranks sharing it): the ``--selftest`` mode counts the
ranks and checks the arg-min exchange, and a rank whose sharded leg dies does not hang the job -- its peers come back from
their collective after ``--dist-timeout``, all ranks agree that the leg failed, and the headline line is still printed
(VERDICT round 3, item 7)."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra, timeout):
    env = dict(os.environ, CUROBO_BENCH_BACKEND="gloo", **env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", *extra], env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


def test_selftest_counts_the_ranks_and_checks_the_exchange(device):
    p, out = _run(["--selftest"], {}, 300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["selftest"] and out["ranks_counted_by_all_reduce"] == 2 and out["global_argmin_ok"]
    assert out["backend"] == "gloo" and out["global_argmin_ms_median"] > 0


def test_a_rank_that_fails_its_leg_does_not_hang_the_job(device):
    # rank 1 raises at the start of the C4 leg; rank 0 is then alone in the leg's collectives until the 20 s timeout
    p, out = _run(["--full", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-ik", "--min-timed-s", "0.02", "--dist-timeout", "20"],
                  {"CUROBO_BENCH_FAIL_LEG": "c4_humanoid_seed_shard:1"}, 600)
    assert out is not None, (p.returncode, p.stderr[-3000:])
    assert out["n_gpus"] == 2 and out["value"] > 0, "the headline is reported"
    assert "value" in out["strong_scaling"] and out["strong_scaling"]["exchange_ms_per_solve"] > 0
    leg = out["multi_gpu_legs"]["c4_humanoid_seed_shard"]
    assert "error" in leg, leg
