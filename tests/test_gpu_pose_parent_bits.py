"""The pose estimators' launches (csrc/pose_detect.hip, csrc/pose_icp.hip, the rules both share in csrc/pose_device.hpp) give the
bits recorded in tests/golden/pose_parent_bits.npz.

The fixture is not a reference's output: it holds what the build BEFORE the shared rules were stated once gave, under this
compiler, on the inputs stored next to it (tests/golden/make_pose_parent_bits.py makes both).  The float64 oracles hold these
kernels inside bounds, which a changed rounding passes; this comparison is exact, on the int32 view of every output word.  A
change that alters arithmetic on purpose re-records the fixture with the script and says so.

SDF evaluate at N = 1 .. 513 (lane, wavefront and workgroup edges, three rows), Huber on and off, points beyond the threshold,
one cloud with no valid point: distance, gradient, valid, every workspace word.  LM step: INIT and two UPDATEs at N = 257, and
one-row workspaces written by hand in both modes (well conditioned, a non-positive pivot, word 0 = +inf, which the LM rule lets
through, a NaN, counts 10 and 11): all 71 state words.  ICP correspond at five (M, O, H), Huber on and off, a finite and an
infinite threshold, one hypothesis stopped with and without honour_stopped: index, distance, every workspace word; the coarse,
fine and finalize steps on those workspaces and on hand-written rows (counts 9 and 10, a non-positive pivot, word 0 = +inf,
which the ICP rule refuses, a solution below the fine stage's translation stop): all 24 state words per hypothesis."""

import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_pose_parent_bits", os.path.join(GOLDEN_DIR, "make_pose_parent_bits.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

INPUTS, WANT = M.load()
RECORDED = sorted(WANT)
GROUPS = sorted({k.split("_")[0] for k in RECORDED})  # sdf, lm, icp


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
