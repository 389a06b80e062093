"""The mesh-obstacle launches (csrc/mesh_bvh.hip, the statements they share in csrc/mesh_device.hpp) give the bits recorded in
tests/golden/mesh_parent_bits.npz.

The fixture is not a reference's output: it holds what the build BEFORE the sweep chain, the sphere staging and the result write
were stated once gave, under this compiler, on the inputs stored next to it (tests/golden/make_mesh_parent_bits.py makes both,
and refuses a file whose cases do not reach the kernels they are there for).  tests/test_gpu_mesh.py holds these kernels to the
oracle inside bounds and to each other "except on ties", which a changed rounding passes; this comparison is exact, on the int32
view of every output word (distance, gradient) and of the four queue counters of every queued launch, which say which kernel
answered how many spheres.  A change that alters arithmetic on purpose re-records the fixture with the script and says so.

world: the mesh world of the collision tests (four live meshes, a disabled slot that shares a BVH), 6 x 5 x 65 spheres (two
select workgroups, the last one ragged; groups beyond the queue's end), as one kernel, queued over meshes without cell lists
(select + tree walk) and queued with cell lists, each with sweep 0, sweep 3, sweep 3 + speed metric, and that with accumulate
onto a non-zero buffer.  ball: 6 x 5 x 16 spheres around the middle of a ball, sweep 0 and 3 (209 of them answered by a
workgroup each).  open: an open box signed by the reference's rays, 2 x 5 x 150 spheres, sweep 0 and 3 (the cell-list kernel hands
every live sphere to the walk through the head of queue2; no sweep culling).  env: two environments with an index
per trajectory, horizon 1 (no neighbour; obstacle slots read per sphere) and 2 (one neighbour; slots staged).  slots: 40 obstacle
slots, the second slot group accumulating onto the first.  gm: gradient_mode 1."""

import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_mesh_parent_bits", os.path.join(GOLDEN_DIR, "make_mesh_parent_bits.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

INPUTS, WANT = M.load()
RECORDED = sorted(WANT)
GROUPS = sorted({k.split("_")[0] for k in RECORDED})  # ball, env, gm, open, slots, world


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
