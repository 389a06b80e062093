"""The decay tests' additions to the scene of tests/mapper_cases.py (50 x 48 x 20 voxels, an 80 x 60 camera): two close cameras
for the frustum test, one turned away from the sphere for the forgetting test, and what the restatement
(tests/mapper_decay_ref.py) says about them.  The conditions the device tests presuppose are asserted in
tests/test_mapper_decay_host.py, where they cost no GPU time."""

import functools

import numpy as np

import mapper_cases as C
import mapper_decay_ref as DR
import mapper_ref as R

BLOCK_SIZES = (2, 4, 8)  # less than a wavefront, exactly one, many per block
#: (eye, target, roll) of the frustum test's two cameras: each sees a corner of the grid from 0.3 .. 0.5 m, so that with the depth
#: range below a good part of the visible blocks is out by the image tests, another by the far bound, and the rest in
FRUSTUM_CAMS = (((0.10, -0.30, 0.30), (0.35, -0.40, -0.15), 0.2), ((-0.10, 0.10, 0.45), (-0.30, 0.35, -0.15), -0.4))
FRUSTUM_DEPTH = (0.1, 0.6)
TIME_DECAY, FRUSTUM_DECAY = 0.97, 0.5
#: the forgetting test's camera: over the +x +y corner, looking down and outward at the ground, the sphere behind it
TURNED = ((0.36, 0.36, 0.2), (0.46, 0.44, -0.15), 0.1)
FORGET_TIME_DECAY = 0.5
SPHERE_BOX = ((-R.SPHERE_RADIUS,) * 3, (R.SPHERE_RADIUS,) * 3)


def cfg_dict(block_size: int = 4) -> dict:
    return {**C.CFG, "block_size": block_size}


@functools.lru_cache(maxsize=None)
def grid(block_size: int = 4) -> "R.Grid":
    from curobo_amd.perception.mapper import MapperCfg

    return R.Grid.from_cfg(MapperCfg(**cfg_dict(block_size)))


def frustum_cameras():
    """(K [2, 3, 3], position [2, 3], quaternion [2, 4]) float32"""
    pos = np.array([c[0] for c in FRUSTUM_CAMS], np.float32)
    quat = np.stack([R.look_at(*c) for c in FRUSTUM_CAMS]).astype(np.float32)
    return np.stack([C.K] * len(FRUSTUM_CAMS)), pos, quat


def frustum_sets(block_size: int):
    """(sure_in, sure_out) of the frustum test's cameras over every block"""
    return DR.frustum_flags(grid(block_size), *frustum_cameras(), C.H, C.W, *FRUSTUM_DEPTH)


@functools.lru_cache(maxsize=None)
def marked(block_size: int):
    """(sure, possible) ever-visible blocks after mapper_cases.FRAMES"""
    g = grid(block_size)
    sure, possible = np.zeros(g.n_blocks, bool), np.zeros(g.n_blocks, bool)
    for cams in C.FRAMES:
        s, p = R.mark_blocks(g, *C.frame(*cams))
        sure, possible = sure | s, possible | p
    return sure, possible


@functools.lru_cache(maxsize=None)
def turned_frame():
    """the turned camera's frame of the sphere scene: (depth [1, H, W], K [1, 3, 3], position [1, 3], quaternion [1, 4])"""
    eye, target, roll = TURNED
    q, pos = R.look_at(eye, target, roll).astype(np.float32), np.asarray(eye, np.float32)
    return R.render_depth(C.K, pos, q, C.H, C.W)[None], C.K[None], pos[None], q[None]


def sphere_blocks() -> np.ndarray:
    """bool [n_blocks]: the blocks (of 4) that touch the sphere's bounding box"""
    return R.blocks_touching(grid(), *SPHERE_BOX)


@functools.lru_cache(maxsize=None)
def forgetting():
    """the restatement's run of the forgetting test: eye 0 once, then the turned camera with time_decay = 0.5 until every block
    the first frame saw and the turned camera does not is recycled, the sphere's among them.  dict(frames: how many turned
    frames that took, states: the per-frame dicts of mapper_decay_ref.frame_sequence)"""
    g = grid()
    states = []

    def frames():
        yield C.frame(0)
        while True:
            yield turned_frame()

    for k, s in enumerate(DR.frame_sequence(g, frames(), FORGET_TIME_DECAY, 1.0, C.H, C.W)):
        states.append(s)
        if k > 0 and not (s["visible"] & ~s["possible"]).any():
            return dict(frames=k, states=states)
        assert k < 64, "the sphere's blocks never go"
