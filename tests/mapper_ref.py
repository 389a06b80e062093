"""Float64 NumPy restatement of the depth mapper's stages (curobo_amd/csrc/mapper.hip), with the reference's file:line next
to each rule (paths under curobo/_src/perception/mapper/).  Same standing as tests/pose_icp_ref.py: the device is compared
with THIS, and this is plain enough to be compared with the reference by reading.

Where float32 and float64 may legitimately decide differently the functions say so instead of deciding: per voxel an
*ambiguous* flag (u or v within 1e-3 px of an integer, z_cam within 1e-5 m of depth_min, sdf within 1e-5 m of -truncation),
per block a *sure* and a *possible* visible set (a block marked only by samples within 1e-4 voxel of a block or grid face is
possible, not sure), per ESDF cell a flag for a probe within 1e-3 voxel of a voxel face or an sdf within 1e-6 m of a seed
threshold."""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

U_TOL, Z_TOL, SDF_TOL, FACE_TOL, PROBE_TOL, SEED_TOL = 1e-3, 1e-5, 1e-5, 1e-4, 1e-3, 1e-6
SDF_INVALID = 1e10  # kernel/wp_tsdf_sample.py SDF_INFINITY as the lookups hand it on (builder_esdf.py:153-158)


@dataclass
class Grid:
    """the TSDF grid: ``nx, ny, nz`` voxels, blocks of ``bs`` voxels per edge, centred on ``origin``"""

    nx: int
    ny: int
    nz: int
    bs: int
    origin: Sequence[float]
    vs: float
    trunc: float
    depth_min: float
    depth_max: float
    min_weight: float

    @property
    def nb(self) -> Tuple[int, int, int]:
        return tuple(-(-n // self.bs) for n in (self.nx, self.ny, self.nz))

    @property
    def n_blocks(self) -> int:
        return int(np.prod(self.nb))

    @property
    def step(self) -> float:
        return self.bs * self.vs / 1.42  # builder_camera_integrate.py: STEP_SIZE

    @property
    def num_samples(self) -> int:
        return int(math.ceil(2.0 * self.trunc / self.step)) + 1  # NUM_SAMPLES

    @classmethod
    def from_cfg(cls, cfg) -> "Grid":
        nz, ny, nx = cfg.grid_shape
        return cls(nx, ny, nz, cfg.block_size, [float(v) for v in cfg.grid_center.tolist()], float(np.float32(cfg.voxel_size)),
                   float(np.float32(cfg.truncation_distance)), float(np.float32(cfg.depth_minimum_distance)),
                   float(np.float32(cfg.depth_maximum_distance)), float(np.float32(cfg.minimum_tsdf_weight)))

    def voxel_centres(self) -> np.ndarray:
        """[n_blocks, bs^3, 3]: block (bx, by, bz) at (bz nby + by) nbx + bx, voxel at lz BS^2 + ly BS + lx (builder_coord.py:163-176),
        centre = origin + (g + 0.5 - N / 2) vs (:57-66); the padding voxels of the last blocks included, as the reference's"""
        nbx, nby, nbz = self.nb
        b = np.arange(self.n_blocks)
        base = np.stack([b % nbx, (b // nbx) % nby, b // (nbx * nby)], -1) * self.bs
        loc = np.arange(self.bs ** 3)
        off = np.stack([loc % self.bs, (loc // self.bs) % self.bs, loc // (self.bs * self.bs)], -1)
        g = base[:, None, :] + off[None, :, :]
        return np.asarray(self.origin) + (g + 0.5 - 0.5 * np.array([self.nx, self.ny, self.nz])) * self.vs


def quat_rotate(q_wxyz: np.ndarray, x: np.ndarray) -> np.ndarray:
    """wp.quat_rotate: x (2 w^2 - 1) + 2 w (v x x) + 2 v (v . x)"""
    w, v = q_wxyz[..., :1], q_wxyz[..., 1:]
    return x * (2.0 * w * w - 1.0) + 2.0 * w * np.cross(v, x) + 2.0 * v * np.sum(v * x, -1, keepdims=True)


def half_steps(a, b) -> np.ndarray:
    """how many fp16 values lie between a and b (0 = equal, 1 = neighbours), for finite fp16 arrays"""
    def order(h):
        bits = np.asarray(h, np.float16).view(np.uint16).astype(np.int32)
        return np.where(bits & 0x8000, -(bits & 0x7fff), bits)
    return np.abs(order(a) - order(b))


# ---------------------------------------------------------------------------------------------------- stage 1: visible blocks
def mark_blocks(g: Grid, depth, K, pos, quat):
    """(sure, possible) bool [n_blocks]  (builder_camera_integrate.py:89-166)"""
    depth, K, pos, quat = (np.asarray(a, np.float64) for a in (depth, K, pos, quat))
    n, H, W = depth.shape
    sure, possible = np.zeros(g.n_blocks, bool), np.zeros(g.n_blocks, bool)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dims = np.array([g.nx, g.ny, g.nz])
    nbx, nby, _ = g.nb
    for c in range(n):
        fx, fy, cx, cy = K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2]                                      # :115-118
        d = depth[c]
        ok = (d >= g.depth_min) & (d <= g.depth_max)                                                          # :121
        edge = (np.abs(d - g.depth_min) < 1e-6) | (np.abs(d - g.depth_max) < 1e-6)
        ray = np.stack([(px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, np.ones_like(d)], -1)                      # :125-127
        z_start = np.maximum(d - g.trunc, g.depth_min)                                                         # :129
        for k in range(g.num_samples):
            z = z_start + k * g.step                                                                           # :130
            margin = z - (d + g.trunc + g.step)
            live = (ok | edge) & (margin <= 1e-6)                                                              # :132
            firm = ok & ~edge & (margin < -1e-6)
            p = pos[c] + quat_rotate(quat[c], ray * z[..., None])                                              # :136-149
            vf = (p - np.asarray(g.origin)) / g.vs + 0.5 * dims                                                # builder_coord.py:45-54
            blocks = []
            for dx in (-FACE_TOL, FACE_TOL):
                for dy in (-FACE_TOL, FACE_TOL):
                    for dz in (-FACE_TOL, FACE_TOL):
                        v = np.floor(vf + np.array([dx, dy, dz])).astype(np.int64)                             # :153-155
                        inside = ((v >= 0) & (v < dims)).all(-1) & live                                        # :157
                        b = ((v[..., 2] // g.bs) * nby + v[..., 1] // g.bs) * nbx + v[..., 0] // g.bs           # :161-164
                        blocks.append(np.where(inside, b, -1))
            blocks = np.stack(blocks, 0)
            for b in blocks:
                possible[b[b >= 0]] = True
            same = (blocks == blocks[0]).all(0) & (blocks[0] >= 0) & firm
            sure[blocks[0][same]] = True
    return sure, possible


# ---------------------------------------------------------------------------------------------------- stage 2: voxels
def integrate(g: Grid, sw, w, visible, depth, K, pos, quat):
    """one frame into the fp16 pair ``sw``, ``w`` [n_blocks, bs^3] over the blocks of ``visible``.  Returns (sw, w) as float16,
    updated bool, ambiguous bool  (builder_camera_integrate.py:400-487)"""
    depth, K, pos, quat = (np.asarray(a, np.float64) for a in (depth, K, pos, quat))
    n, H, W = depth.shape
    centre = g.voxel_centres()                                                                                # :432-437
    tot_sw, tot_w = np.zeros(centre.shape[:2]), np.zeros(centre.shape[:2])
    amb = np.zeros(centre.shape[:2], bool)
    for c in range(n):
        conj = quat[c] * np.array([1.0, -1.0, -1.0, -1.0])                                                     # :454 quat_inverse
        v = quat_rotate(conj, centre - pos[c])                                                                 # :455
        z = v[..., 2]
        front = z > g.depth_min                                                                                # :458
        near = z > g.depth_min - Z_TOL
        zs = np.where(near, z, 1.0)
        fx, fy = K[c, 0, 0], K[c, 1, 1]
        u, vv = fx * v[..., 0] / zs + K[c, 0, 2], fy * v[..., 1] / zs + K[c, 1, 2]                             # :464-465
        px, py = np.trunc(u).astype(np.int64), np.trunc(vv).astype(np.int64)                                   # :467-468 toward zero
        inb = (px >= 0) & (px < W) & (py >= 0) & (py < H)                                                      # :470
        d = depth[c][np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)]
        d_ok = (d >= g.depth_min) & (d <= g.depth_max)                                                         # :472
        sdf = d - z                                                                                            # :473
        keep = front & inb & d_ok & (sdf >= -g.trunc)                                                          # :474
        weight = np.maximum((fx * g.vs / zs) * (fy * g.vs / zs), 1.0)                                          # :476-478, weight fn = 1
        tot_sw += np.where(keep, np.minimum(sdf, g.trunc) * weight, 0.0)                                       # :475, :480
        tot_w += np.where(keep, weight, 0.0)                                                                   # :481
        amb |= near & ((np.abs(z - g.depth_min) < Z_TOL) | (np.abs(u - np.rint(u)) < U_TOL) | (np.abs(vv - np.rint(vv)) < U_TOL)
                       | (inb & d_ok & (np.abs(sdf + g.trunc) < SDF_TOL)))
    upd = (tot_w > 0.0) & np.asarray(visible, bool)[:, None]                                                   # :483, :421-426
    sw64, w64 = np.asarray(sw, np.float16).astype(np.float64), np.asarray(w, np.float16).astype(np.float64)
    new_sw = np.where(upd, sw64 + tot_sw, sw64).astype(np.float16)                                             # :484-487
    new_w = np.where(upd, w64 + tot_w, w64).astype(np.float16)
    return new_sw, new_w, upd, amb


# ---------------------------------------------------------------------------------------------------- TSDF sample
def tsdf_sample(g: Grid, sw, w, block_visible, world):
    """(sdf, probe-ambiguous) at world positions [..., 3]: SDF_INVALID outside the grid, in a block never visible, or unobserved
    (builder_esdf.py:279-300, wp_tsdf_sample.py:46-52)"""
    dims = np.array([g.nx, g.ny, g.nz])
    gf = (world - np.asarray(g.origin)) / g.vs + 0.5 * dims
    gi = np.trunc(gf).astype(np.int64)                                                                         # :279-281 wp.int32()
    amb = (np.abs(gf - np.rint(gf)) < PROBE_TOL).any(-1)
    inside = ((gi >= 0) & (gi < dims)).all(-1)                                                                 # :282
    gc = np.clip(gi, 0, dims - 1)
    nbx, nby, _ = g.nb
    b = ((gc[..., 2] // g.bs) * nby + gc[..., 1] // g.bs) * nbx + gc[..., 0] // g.bs                            # :285-287
    loc = ((gc[..., 2] % g.bs) * g.bs + gc[..., 1] % g.bs) * g.bs + gc[..., 0] % g.bs                           # :293-296
    wv = np.asarray(w, np.float16).astype(np.float64)[b, loc]
    sv = np.asarray(sw, np.float16).astype(np.float64)[b, loc]
    valid = inside & np.asarray(block_visible, bool)[b] & (wv > g.min_weight)                                  # :289-291, ws:49
    return np.where(valid, sv / np.where(valid, wv, 1.0), SDF_INVALID), amb


def esdf_centres(shape, origin, vs) -> np.ndarray:
    """[D, H, W, 3]  (builder_esdf.py:334-336: x is the slowest axis, of D cells)"""
    ax = [(np.arange(n) + 0.5 - 0.5 * n) * vs + o for n, o in zip(shape, origin)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


# ---------------------------------------------------------------------------------------------------- ESDF stage 1: seed
def seed(g: Grid, sw, w, block_visible, shape, esdf_origin, esdf_vs):
    """(seed bool [D, H, W], ambiguous bool)  (builder_esdf.py:267-406)"""
    c = esdf_centres(shape, esdf_origin, esdf_vs)
    out, amb = np.zeros(shape, bool), np.zeros(shape, bool)
    half = 0.5 * esdf_vs                                                                                       # :332
    for off in ((0, 0, 0), (half, 0, 0), (-half, 0, 0), (0, half, 0), (0, -half, 0), (0, 0, half), (0, 0, -half)):  # :338-406
        sdf, a = tsdf_sample(g, sw, w, block_visible, c + np.array(off))
        ok = sdf < 1e9                                                                                         # :299
        out |= ok & ((np.abs(sdf) <= 0.9 * g.vs) | (sdf < -(g.trunc - 1.1 * g.vs)))                            # :302-305
        amb |= a | (ok & ((np.abs(np.abs(sdf) - 0.9 * g.vs) < SEED_TOL) | (np.abs(sdf + (g.trunc - 1.1 * g.vs)) < SEED_TOL)))
    return out, amb


# ---------------------------------------------------------------------------------------------------- ESDF stage 2: nearest site
NO_SITE = np.int64(1) << 40


def edt(seed_mask: np.ndarray):
    """exact squared Euclidean distance (in cells) of every cell to its nearest seed, and that seed: (d2 int64 [D, H, W] with -1
    where there is no seed at all, site int64 [D, H, W, 3]).  Three separable passes, z then y then x: within a pass the site of
    the line's cell j has j as its coordinate along the line, so the pass is min_j (d2(j) + (i - j)^2)."""
    shape = seed_mask.shape
    d2 = np.where(seed_mask, np.int64(0), NO_SITE)
    site = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).astype(np.int64)
    for axis in (2, 1, 0):
        n = shape[axis]
        cost = np.moveaxis(d2, axis, -1)
        i = np.arange(n)
        total = cost[..., None, :] + ((i[:, None] - i[None, :]) ** 2).astype(np.int64)   # [..., i, j]
        j = total.argmin(-1)                                                             # lowest j on a tie
        d2 = np.moveaxis(np.take_along_axis(total, j[..., None], -1)[..., 0], -1, axis)
        s = np.moveaxis(site, axis, -2)                                                  # [..., j, 3]
        site = np.moveaxis(np.take_along_axis(s, j[..., None], -2), -2, axis)
    none = d2 >= NO_SITE
    return np.where(none, -1, d2), np.where(none[..., None], -1, site)


def edt_brute(seed_mask: np.ndarray) -> np.ndarray:
    """d2 by comparing every cell with every seed"""
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in seed_mask.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    seeds = cells[seed_mask.reshape(-1)]
    if len(seeds) == 0:
        return np.full(seed_mask.shape, -1, np.int64)
    out = np.empty(len(cells), np.int64)
    for lo in range(0, len(cells), 2048):
        out[lo:lo + 2048] = ((cells[lo:lo + 2048, None, :] - seeds[None, :, :]) ** 2).sum(-1).min(-1)
    return out.reshape(seed_mask.shape)


def pack_sites(site: np.ndarray) -> np.ndarray:
    """x | y << 10 | z << 20, -1 where there is none"""
    return np.where(site[..., 0] < 0, -1, site[..., 0] | (site[..., 1] << 10) | (site[..., 2] << 20)).astype(np.int32)


def unpack_sites(packed: np.ndarray) -> np.ndarray:
    p = np.asarray(packed, np.int64)
    s = np.stack([p & 0x3ff, (p >> 10) & 0x3ff, (p >> 20) & 0x3ff], -1)
    return np.where(p[..., None] < 0, -1, s)


# ---------------------------------------------------------------------------------------------------- ESDF stage 3: distance
def distance(g: Grid, sw, w, block_visible, d2, esdf_origin, esdf_vs):
    """(fp16 [D, H, W], inside bool)  (builder_esdf.py:412-491, without the skip_steps branch: it reads the static channel only)"""
    sdf, _ = tsdf_sample(g, sw, w, block_visible, esdf_centres(d2.shape, esdf_origin, esdf_vs))               # :474-482
    inside = (sdf < 1e9) & (sdf < 0.0)                                                                         # :484-489
    dist = np.sqrt(np.maximum(d2, 0).astype(np.float64)) * esdf_vs                                             # :442-446
    dist = np.where(d2 < 0, 1e4, np.where(inside, -dist, dist))                                                # :433-435
    return dist.astype(np.float16), inside & (d2 >= 0)


def esdf(g: Grid, sw, w, block_visible, shape, esdf_origin, esdf_vs):
    """the three stages: dict(seed, ambiguous, d2, site, distance)"""
    s, amb = seed(g, sw, w, block_visible, shape, esdf_origin, esdf_vs)
    d2, site = edt(s)
    dist, inside = distance(g, sw, w, block_visible, d2, esdf_origin, esdf_vs)
    return {"seed": s, "ambiguous": amb, "d2": d2, "site": site, "distance": dist, "inside": inside}


# ---------------------------------------------------------------------------------------------------- occupied voxels
def occupied(g: Grid, sw, w, block_visible, surface_only=False, sdf_threshold=None):
    """bool [n_blocks, bs^3]  (builder_raycast.py:1015-1042)"""
    thr = g.vs if sdf_threshold is None else sdf_threshold
    wv, sv = np.asarray(w, np.float16).astype(np.float64), np.asarray(sw, np.float16).astype(np.float64)
    valid = np.asarray(block_visible, bool)[:, None] & (wv > g.min_weight)
    sdf = sv / np.where(valid, wv, 1.0)
    return valid & ((np.abs(sdf) < thr) if surface_only else (sdf <= 0.0))


def blocks_touching(g: Grid, lo, hi) -> np.ndarray:
    """bool [n_blocks]: the blocks a world-space box touches"""
    dims = np.array([g.nx, g.ny, g.nz])
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    b0 = np.floor(((np.asarray(lo, np.float64) - np.asarray(g.origin)) / g.vs + 0.5 * dims) / g.bs).astype(np.int64)
    b1 = np.floor(((np.asarray(hi, np.float64) - np.asarray(g.origin)) / g.vs + 0.5 * dims) / g.bs).astype(np.int64)
    nbx, nby, nbz = g.nb
    b = np.arange(g.n_blocks)
    c = np.stack([b % nbx, (b // nbx) % nby, b // (nbx * nby)], -1)
    return ((c >= b0) & (c <= b1)).all(-1)


# ---------------------------------------------------------------------------------------------------- the test scene
SPHERE_RADIUS = 0.25
GROUND_Z = -0.15


def look_at(eye, target, roll: float) -> np.ndarray:
    """wxyz quaternion of a camera at ``eye`` whose +z looks at ``target``, rolled about its axis"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross(zc, [0.0, 0.0, 1.0])
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    c, s = math.cos(roll), math.sin(roll)
    R = np.stack([c * xc + s * yc, -s * xc + c * yc, zc], 1)  # columns: the camera's axes in the world
    w = 0.5 * math.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12))
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def render_depth(K, pos, quat, H: int, W: int, radius: float = SPHERE_RADIUS, ground_z: float = GROUND_Z, holes=None) -> np.ndarray:
    """z-depth (float32, metres, 0 = nothing) of a sphere at the origin over the plane z = ground_z, through pixel centres"""
    K, pos, quat = (np.asarray(a, np.float64) for a in (K, pos, quat))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray_c = np.stack([(px + 0.5 - K[0, 2]) / K[0, 0], (py + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    ray = quat_rotate(quat, ray_c)  # world direction per unit of camera z
    a, b, c = (ray * ray).sum(-1), 2.0 * (ray * pos).sum(-1), (pos * pos).sum() - radius * radius
    disc = b * b - 4 * a * c
    t_s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t_s = np.where(t_s > 0, t_s, np.inf)
    t_p = np.where(ray[..., 2] < -1e-9, (ground_z - pos[2]) / np.where(ray[..., 2] < -1e-9, ray[..., 2], -1.0), np.inf)
    t_p = np.where(t_p > 0, t_p, np.inf)
    t = np.minimum(t_s, t_p)
    depth = np.where(np.isfinite(t), t, 0.0).astype(np.float32)
    if holes is not None:
        depth[holes] = 0.0
    return depth


def scene_distance(p: np.ndarray, radius: float = SPHERE_RADIUS, ground_z: float = GROUND_Z) -> np.ndarray:
    """distance of world points to the nearer of the sphere and the ground"""
    return np.minimum(np.linalg.norm(p, axis=-1) - radius, p[..., 2] - ground_z)
