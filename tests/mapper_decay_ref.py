"""Restatement of the mapper's weight decay and block recycling (curobo_amd/csrc/mapper.hip: mapper_decay_*_kernel), in the style
of tests/mapper_ref.py: the reference's file:line next to each rule (paths under curobo/_src/perception/mapper/).  The device is
compared with THIS.

Three kinds of statement, each as exact as it can be:
  * the frustum flags in float64, with a *sure in* / *sure out* / *either* answer per block: a block is *either* when a quantity
    the rule compares lies within a tolerance of its bound (mapper_ref's constants: Z_TOL = 1e-5 m for the two depth tests and
    ``z_cam < 0.01``, U_TOL = 1e-3 px for the four image tests), where float32 and float64 may decide differently;
  * the decay arithmetic with torch on the CPU, in exactly the reference's two expressions, so that the stored words are compared
    bit for bit;
  * the block sums in float64: a block is *either* at the recycle threshold when its sum is within SUM_TOL = 1e-4 relative of it
    (an fp32 sum of up to 32768 fp16 weights in any order is within 2e-6 relative of the float64 one).
"""

from __future__ import annotations

import numpy as np
import torch

import mapper_ref as R

SUM_TOL = 1e-4
REFERENCE_BLOCK_SIZE = 8                  # constants.py:55
REFERENCE_BLOCK_EMPTY_THRESHOLD = 0.01    # kernel/builder/builder_decay.py:69
SPHERE_FACTOR = float(np.float32(0.866))  # builder_decay.py:168, a float32 literal in the kernel


def empty_threshold(block_size: int) -> float:
    """builder_decay.py:103-105"""
    return REFERENCE_BLOCK_EMPTY_THRESHOLD * float(block_size ** 3) / float(REFERENCE_BLOCK_SIZE ** 3)


def block_centres(g: "R.Grid") -> np.ndarray:
    """[n_blocks, 3]: ((b BS + BS / 2) - GRID / 2) voxel_size + origin per axis, block (bx, by, bz) at (bz nby + by) nbx + bx
    (builder_decay.py:154-165; there bx = key + blocks // 2, the dense index)"""
    nbx, nby, _ = g.nb
    b = np.arange(g.n_blocks)
    c = np.stack([b % nbx, (b // nbx) % nby, b // (nbx * nby)], -1).astype(np.float64)
    return (c * g.bs + 0.5 * g.bs - 0.5 * np.array([g.nx, g.ny, g.nz])) * g.vs + np.asarray(g.origin, np.float64)


def camera_flags(centres, bs, vs, K, pos, quat, H, W, depth_min, depth_max):
    """one camera: (inside bool, either bool) per block centre  (builder_decay.py:167-215)"""
    K, pos, quat = (np.asarray(a, np.float64) for a in (K, pos, quat))
    r = SPHERE_FACTOR * (bs * vs)                                                                              # :167-168
    v = R.quat_rotate(quat * np.array([1.0, -1.0, -1.0, -1.0]), np.asarray(centres, np.float64) - pos)         # :181-183 quat_inverse
    z = v[..., 2]                                                                                              # :185
    out_depth = (z + r < depth_min) | (z - r > depth_max)                                                      # :186-189
    amb = (np.abs(z + r - depth_min) < R.Z_TOL) | (np.abs(z - r - depth_max) < R.Z_TOL)
    behind = z < 0.01                                                                                          # :191-193
    amb |= ~out_depth & (np.abs(z - 0.01) < R.Z_TOL)
    zs = np.where(behind, 1.0, z)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]                                                        # :195-198
    u, w = fx * v[..., 0] / zs + cx, fy * v[..., 1] / zs + cy                                                  # :200-201
    ru, rw = fx * r / zs, fy * r / zs                                                                          # :203-204
    tests = np.stack([u + ru, u - ru - W, w + rw, w - rw - H], -1)
    out_image = (tests[..., 0] < 0.0) | (tests[..., 1] > 0.0) | (tests[..., 2] < 0.0) | (tests[..., 3] > 0.0)  # :206-213
    amb |= ~out_depth & ~behind & (np.abs(tests) < R.U_TOL).any(-1)
    inside = ~out_depth & (behind | ~out_image)
    return inside, amb


def frustum_flags(g: "R.Grid", K, pos, quat, H: int, W: int, depth_min: float, depth_max: float):
    """the union over the cameras (the flag is set by any of them, builder_decay.py:124-131): (sure_in, sure_out) bool [n_blocks];
    a block in neither is *either*.  K [n, 3, 3], pos [n, 3], quat [n, 4] wxyz"""
    centres = block_centres(g)
    dmin, dmax = float(np.float32(depth_min)), float(np.float32(depth_max))  # (kernel arguments are float32)
    sure_in, sure_out = np.zeros(g.n_blocks, bool), np.ones(g.n_blocks, bool)
    for c in range(len(K)):
        inside, amb = camera_flags(centres, g.bs, g.vs, K[c], pos[c], quat[c], H, W, dmin, dmax)
        sure_in |= inside & ~amb
        sure_out &= ~inside & ~amb
    return sure_in, sure_out


# ---------------------------------------------------------------------------------------------------- the arithmetic, bit for bit
def _tensor(data) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(np.asarray(data, np.float16)).copy())


def decay_uniform(data, factor: float) -> np.ndarray:
    """fp16 [n_blocks, bs^3, 2] times a Python scalar, left alone when the scalar is >= 1  (wp_decay.py:48-49, :124-127)"""
    t = _tensor(data)
    if factor < 1.0:
        t.mul_(factor)
    return t.numpy()


def decay_frustum(data, in_frustum, time_decay: float, frustum_decay: float) -> np.ndarray:
    """the per-block factor tensor is fp16 (storage.py:390), filled with time_decay and, in the frustum, with the Python product
    time_decay * frustum_decay; then block_data.mul_(factor)  (wp_decay.py:136-141)"""
    t = _tensor(data)
    n = t.shape[0]
    factor = torch.empty(n, dtype=torch.float16)
    factor.fill_(time_decay)
    factor.masked_fill_(torch.from_numpy(np.asarray(in_frustum, bool)), time_decay * frustum_decay)
    t.mul_(factor.view(n, 1, 1))
    return t.numpy()


# ---------------------------------------------------------------------------------------------------- recycling
def recycle(data, visible, block_size: int):
    """(data, visible, recycled, either) after the recycle launch: an allocated block whose weights sum to less than the threshold
    is freed (wp_decay.py:54-56 / :147, builder_decay.py:346-363; this mapper has no static channel), its words zero when it is
    allocated again (builder_hash.py:474-492), which the dense storage does at once"""
    data, visible = np.array(data, np.float16), np.asarray(visible, bool)
    sums = data[..., 1].astype(np.float64).sum(1)
    thr = empty_threshold(block_size)
    recycled = visible & (sums < thr)                                                                          # :355
    either = visible & (np.abs(sums - thr) <= SUM_TOL * thr)
    data[recycled] = 0
    return data, visible & ~recycled, recycled, either


def step_uniform(data, visible, block_size: int, factor: float):
    """decay_and_recycle(tsdf, factor)  (wp_decay.py:28-59)"""
    return recycle(decay_uniform(data, factor), visible, block_size)


def step_frame(data, visible, block_size: int, in_frustum, time_decay: float, frustum_decay: float):
    """the frame decay (integrator_tsdf.py:611-675 -> wp_decay.py:111-149): the uniform expression when frustum_decay >= 1"""
    if frustum_decay >= 1.0:
        return step_uniform(data, visible, block_size, time_decay)
    return recycle(decay_frustum(data, in_frustum, time_decay, frustum_decay), visible, block_size)


def frame_sequence(g: "R.Grid", frames, time_decay: float, frustum_decay: float, H: int, W: int):
    """the per-frame sequence from an empty map (integrator_tsdf.py integrate): decay -- not before the first frame (:617), not
    with both factors >= 1 (:619) --, then mark, then integrate.  ``frames``: (depth, K, pos, quat) stacks per frame.  The
    oracle integrates a frame's SURE blocks and takes a block that is *either* in the frustum test as outside; yields per frame
    dict(sw, w, visible, recycled, either_frustum, either_sum, sure, possible, updated, ambiguous)."""
    n, v = g.n_blocks, g.bs ** 3
    data, visible = np.zeros((n, v, 2), np.float16), np.zeros(n, bool)
    for k, f in enumerate(frames):
        depth, K, pos, quat = f
        recycled = either_f = either_s = np.zeros(n, bool)
        if k > 0 and (time_decay < 1.0 or frustum_decay < 1.0):
            sure_in, sure_out = frustum_flags(g, K, pos, quat, H, W, g.depth_min, g.depth_max)
            either_f = visible & ~(sure_in | sure_out) & (frustum_decay < 1.0)
            data, visible, recycled, either_s = step_frame(data, visible, g.bs, sure_in, time_decay, frustum_decay)
        sure, possible = R.mark_blocks(g, depth, K, pos, quat)
        sw, w, upd, amb = R.integrate(g, data[..., 0], data[..., 1], sure, depth, K, pos, quat)
        data, visible = np.stack([sw, w], -1), visible | sure
        yield dict(sw=sw, w=w, visible=visible.copy(), recycled=recycled, either_frustum=either_f, either_sum=either_s, sure=sure,
                   possible=possible, updated=upd, ambiguous=amb)
