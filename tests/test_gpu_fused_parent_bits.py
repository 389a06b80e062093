"""The launches on the device machinery of csrc/fused_device.hpp -- the fused trajectory rollout (csrc/rollout_fused.hip,
csrc/rollout_fused_shape.hip), the one-launch IK rollout (csrc/rollout_ik_fused.hip) and the PRM planner's steering
(csrc/graph_planner.hip) -- give the bits recorded in tests/golden/fused_parent_bits.npz.

The fixture is not a reference's output: it holds what the build BEFORE the row FK of a point, the row arg-max of the staged pair
list, the walk over the lane-dealt pair lists, the sphere-per-lane scene pass and the arg-max key's decoding were stated once gave,
under this compiler, on the inputs that tests/golden/make_fused_parent_bits.py builds (and refuses to record unless every case
reaches the copy it is there for).  The parity tests (tests/test_gpu_fused.py, test_gpu_ik.py, test_gpu_graph_planner.py) hold
these kernels to the kernel sequence and the oracle inside bounds, which a changed rounding or a changed tie rule passes; this
comparison is exact, on the int32 view of every output word.  A change that alters arithmetic on purpose re-records the fixture
with the script and says so.

traj: Franka, 24 trajectories with the knots scaled by 1.6 -- one leftover point (padded horizon 33), none (31) and three (67),
each with the lane-dealt pair lists and with the row form, self collision only and self + swept scene collision with the speed
metric; the generic instantiation of the same launch; the 37-cuboid world (sphere-per-lane scene pass of a row), a cuboid + ESDF
grid world, a world of analytic primitives; one trajopt launch with the pose and c-space terms.  ik: 64 configurations on
cuboids, cuboids + grid, a grid alone, and two environments with their own sphere sets.  steer: 32 edges through the C2 world
(early stop, end reached, infeasible start) and 40 configurations in point mode (a ragged last workgroup)."""

import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_fused_parent_bits", os.path.join(GOLDEN_DIR, "make_fused_parent_bits.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

INPUTS, WANT = M.load()
RECORDED = sorted(WANT)
GROUPS = sorted({k.split("_")[0] for k in RECORDED})  # ik, steer, traj


@pytest.fixture(scope="module")
def replayed():
    return M.replay(INPUTS)


@pytest.mark.parametrize("group", GROUPS)
def test_every_word_is_the_recorded_one(replayed, group):
    names = [k for k in RECORDED if k.startswith(group + "_")]
    assert names and sorted(replayed) == RECORDED
    differing = {}
    for k in names:
        got, want = replayed[k], WANT[k]
        assert got.dtype == want.dtype == np.int32 and got.shape == want.shape, k
        if not np.array_equal(got, want):
            differing[k] = int((got != want).sum())
    print(f"{group}: {len(names)} arrays, {sum(WANT[k].size for k in names)} words, differing: {differing or 'none'}")
    assert not differing
