"""Voxel-grid scene-collision cases at the edges of the lookup (test infrastructure, host side, numpy only).

``stack_voxel_grids`` assembles several grids per environment into one store; the padding of the feature rows and every
slot a kernel must not read (slot >= count, disabled slot) hold -1.0, "deep inside": a read past a grid's own voxels or
past the count shows up as a collision.  ``family(name)`` returns the named cases as ``VoxelCase``s; every family except
``step`` and ``extremes`` is checked to be 1-Lipschitz up to fp16 rounding, which the kernel's culls rely on (as
tests/test_scene_primitives.py notes for primitives).

Where a floor, a truncation or a validity test decides, the queries either sit EXACTLY on the surface in arithmetic that is
exact in float32 and float64 alike (voxel size 2^-4, quarter-voxel lattice, identity rotation, translations on the lattice)
or stay 1/16 voxel away from it (rotated poses), so a float64 restatement and a float32 kernel take the same branch.
"""

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import voxel_ref as VR

VS = 0.0625  # voxel size: a power of two
POISON = -1.0
FAMILIES = ("thin", "shell", "pose", "store", "truncated", "extremes", "sweep", "coarse", "step")
NOT_LIPSCHITZ = ("extremes", "step")


@dataclass
class VoxelCase:
    name: str
    arrays: dict
    spheres: np.ndarray  # [B, H, S, 4] float32
    eta: float
    weight: float
    env: Optional[np.ndarray] = None  # [B] int32: environment of every batch row (None: one environment)
    lipschitz: bool = True
    info: dict = field(default_factory=dict)

    @property
    def multi_env(self):
        return self.env is not None


# ------------------------------------------------------------------------------------------------ poses and grids
def _quat_rotate(q_wxyz, v):
    w, x, y, z = q_wxyz
    qv = np.array([x, y, z], np.float64)
    t = 2.0 * np.cross(qv, v)
    return v + w * t + np.cross(qv, t)


def inverse_pose8(pose7):
    """[x y z qw qx qy qz] -> the store's inverse pose [x y z qw qx qy qz pad] (float32)"""
    p, q = np.asarray(pose7[:3], np.float64), np.asarray(pose7[3:7], np.float64)
    q = q / np.linalg.norm(q)
    qi = np.array([q[0], -q[1], -q[2], -q[3]])
    out = np.zeros(8, np.float32)
    out[:3], out[3:7] = -_quat_rotate(qi, p), qi
    return out


def grid_to_world(pose7, lp):
    q = np.asarray(pose7[3:7], np.float64)
    return _quat_rotate(q / np.linalg.norm(q), np.asarray(lp, np.float64)) + np.asarray(pose7[:3], np.float64)


def voxel_centres(shape, vs=VS):
    ax = [(np.arange(n) + 0.5 - n / 2.0) * vs for n in shape]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def ball(c, r):
    return lambda p: np.linalg.norm(p - np.asarray(c, np.float64), axis=-1) - r


def union(*fields):
    return lambda p: np.minimum.reduce([f(p) for f in fields])


def make_grid(shape, pose7=(0, 0, 0, 1, 0, 0, 0), field_local=None, values=None, vs=VS, enable=True, clip=None):
    """one grid: ``field_local`` (grid frame) sampled at the voxel centres, or explicit ``values`` [nx, ny, nz]"""
    shape = tuple(int(v) for v in shape)
    v = np.asarray(values, np.float64).reshape(-1) if values is not None else field_local(voxel_centres(shape, vs))
    if clip is not None:
        v = np.minimum(v, clip)
    assert v.size == shape[0] * shape[1] * shape[2]
    return {"shape": shape, "voxel_size": float(vs), "pose": tuple(float(x) for x in pose7), "values": v.astype(np.float16),
            "enable": bool(enable)}


def poison_grid(enable=True):
    """a slot no kernel may read: 4^3 voxels of half a metre around the origin, all "deep inside" """
    return make_grid((4, 4, 4), values=np.full(64, POISON), vs=0.5, enable=enable)


def stack_voxel_grids(envs, max_distance=10000.0, n_slots=None):
    """``envs[e]`` = the grids of environment e (``make_grid``), in slot order -> the store: voxel_params [E, n, 4],
    voxel_inv_pose [E, n, 8], voxel_enable [E, n], voxel_count [E], voxel_features fp16 [E, n, nvox, 1] padded to the largest
    grid.  Slots >= count are enabled poison grids, the padding of every feature row is -1.0."""
    E = len(envs)
    n = n_slots or max(len(g) for g in envs)
    filled = [list(g) + [poison_grid()] * (n - len(g)) for g in envs]
    nvox = max(int(np.prod(g["shape"])) for gs in filled for g in gs)
    prm = np.zeros((E, n, 4), np.float32)
    inv = np.zeros((E, n, 8), np.float32)
    en = np.zeros((E, n), np.uint8)
    feats = np.full((E, n, nvox, 1), POISON, np.float16)
    for e, gs in enumerate(filled):
        for o, g in enumerate(gs):
            prm[e, o] = [*g["shape"], g["voxel_size"]]
            inv[e, o] = inverse_pose8(g["pose"])
            en[e, o] = 1 if g["enable"] else 0
            feats[e, o, : g["values"].size, 0] = g["values"]
    return {"voxel_params": prm, "voxel_inv_pose": inv, "voxel_enable": en, "voxel_count": np.array([len(g) for g in envs], np.int32),
            "voxel_features": feats, "voxel_max_distance": float(max_distance)}


def with_far_cuboids(arrays, k):
    """the same store plus ``k`` small enabled cuboids 50 m away (they touch nothing; they only add obstacle records)"""
    E = arrays["voxel_params"].shape[0]
    dims = np.zeros((E, k, 4), np.float32)
    dims[..., :3] = 0.1
    inv = np.zeros((E, k, 8), np.float32)
    inv[..., 3] = 1.0
    inv[..., 0] = -(50.0 + np.arange(k))
    inv[..., 1] = inv[..., 2] = -50.0
    return {**arrays, "cuboid_dims": dims, "cuboid_inv_pose": inv, "cuboid_enable": np.ones((E, k), np.uint8),
            "cuboid_count": np.full((E,), k, np.int32)}


def assert_lipschitz(grid):
    """neighbouring voxels (26-neighbourhood) differ by at most their distance, up to fp16 rounding of both values"""
    v = grid["values"].astype(np.float64).reshape(grid["shape"])
    vs = grid["voxel_size"]
    for off in [(a, b, c) for a in (0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]:
        sl_a, sl_b = [], []
        for d, n in zip(off, v.shape):
            sl_a.append(slice(max(d, 0), n + min(d, 0)))
            sl_b.append(slice(max(-d, 0), n + min(-d, 0)))
        a, b = v[tuple(sl_a)], v[tuple(sl_b)]
        if a.size == 0:
            continue
        bound = np.linalg.norm(off) * vs * (1 + 1e-9) + 2.0 ** -11 * (np.abs(a) + np.abs(b)) + 1e-7
        assert (np.abs(a - b) <= bound).all(), (grid["shape"], off, float((np.abs(a - b) - bound).max()))


# ------------------------------------------------------------------------------------------------ query sets
def lattice(shape, margin=1.5, step=0.25, shift=0.0, vs=VS):
    """grid-frame points on a ``step``-voxel lattice from ``margin`` voxels outside every face (``shift`` voxels off it)"""
    ax = [(np.arange(-(n / 2.0 + margin), n / 2.0 + margin + 1e-9, step) + shift) * vs for n in shape]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _layout(points, radii, h=8, s=4):
    """[N, 3] points -> [B, h, s, 4]; N is cut to a multiple of h * s (the callers put what must stay first)"""
    n = (len(points) // (h * s)) * h * s
    sph = np.concatenate([points[:n], np.resize(np.asarray(radii, np.float64), n)[:, None]], -1)
    return sph.reshape(-1, h, s, 4).astype(np.float32)


def _stratified(rng, classes, per_class):
    keep = []
    for c in np.unique(classes):
        idx = np.nonzero(classes == c)[0]
        keep.append(rng.choice(idx, min(per_class, len(idx)), replace=False))
    return np.concatenate(keep)


def _shell_like(name, rng, pose_a, pose_b, shift, eta=0.02, weight=1.0):
    """grids (5, 4, 3) and (6, 6, 6); queries 1.5 voxels outside to 1.5 voxels inside every face, edge and corner, stratified
    by the number of valid corners, plus the voxel centres (fx = 0)"""
    shapes, poses = [(5, 4, 3), (6, 6, 6)], [pose_a, pose_b]
    grids, pts, cls = [], [], []
    for shape, pose in zip(shapes, poses):
        corner = np.asarray(shape) * VS / 2.0
        g = make_grid(shape, pose, union(ball(corner, 2 * VS), ball((0, 0, 0), VS)))
        assert_lipschitz(g)
        grids.append(g)
        lat = lattice(shape, shift=shift)
        inner = (np.abs(lat) < (np.asarray(shape) / 2.0 - 1.5) * VS - 1e-9).all(-1)  # deeper than 1.5 voxels inside: not the shell
        lat = lat[~inner]
        c = VR.valid_corner_count([*shape, VS], lat)
        take = _stratified(rng, c, 420)
        centres = voxel_centres(shape) + shift * VS
        lp = np.concatenate([centres, lat[take]])
        pts.append(grid_to_world(pose, lp))
        cls.append(np.concatenate([VR.valid_corner_count([*shape, VS], centres), c[take]]))
    arrays = stack_voxel_grids([grids], max_distance=10.0)
    order = rng.permutation(sum(len(p) for p in pts))
    points, classes = np.concatenate(pts)[order], np.concatenate(cls)[order]
    sph = _layout(points, [0.013, 0.0291, 0.047])
    classes = classes[: sph[..., 0].size].reshape(sph.shape[:3])
    case = VoxelCase(name, arrays, sph, eta, weight, info={"classes": classes})
    ref = VR.scene_collision(sph, arrays, weight, eta)
    for k in (0, 1, 2, 4, 8):
        assert (classes == k).sum() >= 20, (name, k, int((classes == k).sum()))
    for k in (1, 2, 4):
        assert ((classes == k) & (ref["distance"] > 0)).any(), f"{name}: no penetrating query with {k} valid corners"
    return case


def _thin(rng):
    shapes = [(1, 4, 5), (4, 1, 5), (4, 5, 1), (1, 1, 1)]
    offs = [(0, 0, 0), (1.0, 0, 0), (0, 1.0, 0), (1.0, 1.0, 0.5)]
    grids, pts = [], []
    for shape, t in zip(shapes, offs):
        g = make_grid(shape, (*t, 1, 0, 0, 0), ball((0.01, 0.02, -0.03), 0.06))
        assert_lipschitz(g)
        grids.append(g)
        lat = lattice(shape)  # from 1.5 voxels outside every face: the index is truncated towards zero, not floored
        low = ((lat < -np.asarray(shape) * VS / 2.0) & (lat > -(np.asarray(shape) / 2.0 + 1.0) * VS)).any(-1)
        take = np.concatenate([rng.choice(np.nonzero(low)[0], 300, replace=False), rng.choice(len(lat), 500, replace=False)])
        pts.append(lat[take] + np.asarray(t))
    points = np.concatenate(pts)[rng.permutation(3200)]
    return VoxelCase("thin", stack_voxel_grids([grids], max_distance=10.0), _layout(points, [0.011, 0.0273, 0.0531]), 0.02, 3.0)


def _truncated(rng, md):
    g = make_grid((8, 8, 8), field_local=ball((0.01, -0.02, 0.0), 0.1), clip=md)
    assert_lipschitz(g)
    lat = lattice((8, 8, 8))
    lp = np.concatenate([voxel_centres((8, 8, 8)), lat[rng.choice(len(lat), 1504, replace=False)]])
    eta = 0.02
    # radii on both sides of max_distance - eta (at and above it the early rejects are off and every sphere collides)
    radii = [md - eta - 0.004, md - eta + 0.004, 0.03, 0.2]
    stored = g["values"].astype(np.float32)
    exact = bool((stored == np.float32(md)).any())
    return VoxelCase(f"truncated_{md}", stack_voxel_grids([[g]], max_distance=md), _layout(lp[rng.permutation(len(lp))], radii), eta, 1.0,
                     info={"stored_reaches_max_distance": exact})


def _extremes(rng):
    tiny = np.array([6e-8, -6e-8, -0.0, 0.0, 2.0 ** -14, 1.2e-7], np.float64)  # fp16 subnormals, zeros, the smallest normal
    v = np.zeros((8, 8, 8))
    # x slabs; +65504 and -65504 never share a cell, so no interpolation cancels two huge terms
    for x, val in enumerate([1e4, 65504.0, 1e4, None, -0.02, -65504.0, -65504.0, -0.03]):
        v[x] = tiny[rng.integers(0, len(tiny), (8, 8))] if val is None else val
    a = make_grid((8, 8, 8), values=v)
    b = make_grid((6, 6, 6), (1.0, 0, 0, 1, 0, 0, 0), values=np.full(216, 1e4))  # nothing seen anywhere: the mapper's value
    la, lb = lattice((8, 8, 8)), lattice((6, 6, 6)) + np.array([1.0, 0, 0])
    lp = np.concatenate([voxel_centres((8, 8, 8)), la[rng.choice(len(la), 1500, replace=False)], lb[rng.choice(len(lb), 300, replace=False)]])
    return VoxelCase("extremes", stack_voxel_grids([[a, b]], max_distance=10000.0), _layout(lp[rng.permutation(len(lp))], [0.013, 0.0291, 0.047]),
                     0.02, 1.0, lipschitz=False, info={"swept_slope": 2 * 65504.0 / VS})


def _step(rng):
    v = np.full((8, 8, 8), 1e4)  # unknown ...
    v[3:5, 2:6, 2:6] = -0.05    # ... next to occupied: not 1-Lipschitz
    g = make_grid((8, 8, 8), values=v)
    lat = lattice((8, 8, 8))
    lp = np.concatenate([voxel_centres((8, 8, 8)), lat[rng.choice(len(lat), 1504, replace=False)]])
    return VoxelCase("step", stack_voxel_grids([[g]], max_distance=10000.0), _layout(lp[rng.permutation(len(lp))], [0.013, 0.0291, 0.047]),
                     0.02, 1.0, lipschitz=False)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _lines(p_mid, direction, step, h=8, h_mid=3):
    """[T, h, 3]: straight trajectories through p_mid at sample h_mid"""
    k = (np.arange(h) - h_mid)[None, :, None]
    return p_mid[:, None, :] + k * step[:, None, None] * direction[:, None, :]


STEPS_VOXELS = (0.2, 1.0, 3.5, 4.0, 8.0)  # (no step below 1e-3 m: spheres that rest up to rounding belong to other tests)


def _sweep(rng):
    half = 6 * VS
    wall = lambda p: 0.30 - p[..., 0]  # noqa: E731  (occupied beyond x = 0.30, reaching the +x face at 0.375)
    g = make_grid((12, 12, 12), field_local=union(ball((0, 0, 0), 0.1), wall))
    assert_lipschitz(g)
    r_of = np.array([0.02, 0.035])
    eta, per = 0.02, 16
    traj, rad = [], []
    for sv in STEPS_VOXELS:
        L = np.full(per, sv * VS)
        # (a) across a face from outside: the +x face (into the wall) and the +y face
        f = np.stack([np.full(per, half), rng.uniform(-0.3, 0.3, per), rng.uniform(-0.3, 0.3, per)], -1)
        d = _unit(rng, per) * 0.4 + np.array([-1.0, 0, 0])
        sw = rng.random(per) < 0.5
        f[sw] = f[sw][:, [1, 0, 2]]
        d[sw] = d[sw][:, [1, 0, 2]]
        traj.append(_lines(f, d / np.linalg.norm(d, axis=-1, keepdims=True), L))
        # (b) along the +x face, from one voxel outside to one voxel inside
        off = rng.choice([-1.0, -0.5, -0.25, 0.25, 0.5, 1.0], per) * VS
        f = np.stack([half + off, rng.uniform(-0.2, 0.2, per), rng.uniform(-0.2, 0.2, per)], -1)
        t = _unit(rng, per)
        t[:, 0] = 0
        traj.append(_lines(f, t / np.linalg.norm(t, axis=-1, keepdims=True), L))
        # (c) past the ball at a centre clearance on both sides of half_step + 3.5 voxels
        rr = r_of[np.arange(per) % 2]
        delta = rng.choice([-1.0, -0.3, 0.3, 1.0], per) * VS
        D = 0.1 + rr + eta + 0.5 * L + 3.5 * VS + delta
        u = _unit(rng, per)
        u[:, 0] = -np.abs(u[:, 0])  # away from the wall
        t = np.cross(u, _unit(rng, per))
        traj.append(_lines(u * D[:, None], t / np.linalg.norm(t, axis=-1, keepdims=True), L))
        rad += [r_of[np.arange(per) % 2]] * 3
    traj, rad = np.concatenate(traj), np.concatenate(rad)  # [T, 8, 3], [T]
    sph = np.concatenate([traj, np.broadcast_to(rad[:, None, None], traj.shape[:2] + (1,))], -1)
    sph = sph.reshape(-1, 4, 8, 4).transpose(0, 2, 1, 3).astype(np.float32)  # four trajectories side by side per batch row
    return VoxelCase("sweep", stack_voxel_grids([[g]], max_distance=10.0), np.ascontiguousarray(sph), eta, 1.0)


def _coarse(rng):
    poses = [(0, 0, 0, 1, 0, 0, 0), (0.75, 0.25, 0, 1, 0, 0, 0)]
    # a ball inside the first grid; a wall 1 cm outside the low-x face of the second: its field is shallow (minimum 0.01), so the
    # block minima sit just below the spheres' r + eta and a cull that compares them carelessly drops real penetrations
    wall = lambda p: p[..., 0] + 3.5 * VS + 0.01  # noqa: E731
    grids = [make_grid((9, 6, 5), poses[0], ball((0.02, 0.0, -0.01), 0.09)), make_grid((8, 8, 8), poses[1], wall)]
    traj = []
    per = 20
    for g in grids:
        assert_lipschitz(g)
        for sv in STEPS_VOXELS:  # half steps of 0.1 .. 4 voxels: sweep reach on both sides of (dilate - 1) = 2 voxels
            mid = rng.uniform(-0.5, 0.5, (per, 3)) * np.asarray(g["shape"]) * VS * 0.9 + np.asarray(g["pose"][:3])
            traj.append(_lines(mid, _unit(rng, per), np.full(per, sv * VS)))
    traj = np.concatenate(traj)
    rad = np.array([0.02, 0.035])[np.arange(len(traj)) % 2]
    sph = np.concatenate([traj, np.broadcast_to(rad[:, None, None], traj.shape[:2] + (1,))], -1)
    sph = sph.reshape(-1, 4, 8, 4).transpose(0, 2, 1, 3).astype(np.float32)
    return VoxelCase("coarse", stack_voxel_grids([grids], max_distance=10.0), np.ascontiguousarray(sph), 0.02, 1.0)


def _store(rng):
    """two environments, three slots: counts 3 and 2, a disabled slot inside the count, different dimensions per slot"""
    f = ball((0.0, 0.01, 0.0), 1.2 * VS)
    env0 = [make_grid((5, 4, 3), (0.25, 0, 0, 1, 0, 0, 0), f), poison_grid(enable=False), make_grid((7, 3, 6), (-0.25, 0.25, 0, 1, 0, 0, 0), f)]
    env1 = [make_grid((4, 6, 5), (0, -0.25, 0.25, 1, 0, 0, 0), f), make_grid((3, 3, 4), (0.25, 0.25, -0.25, 1, 0, 0, 0), f)]
    for g in (env0[0], env0[2], *env1):
        assert_lipschitz(g)
    arrays = stack_voxel_grids([env0, env1], max_distance=10.0)
    assert arrays["voxel_count"].tolist() == [3, 2] and arrays["voxel_params"].shape[1] == 3
    real = [[env0[0], env0[2]], env1]
    cases = []
    for b, h, s in [(5, 17, 3), (8, 8, 4), (1, 257, 1), (9, 37, 1)]:  # 255, 256, 257 spheres; horizon * spheres = 37
        env = (np.arange(b) % 2).astype(np.int32) if b > 1 else np.array([1], np.int32)
        sph = np.zeros((b, h, s, 4), np.float32)
        for row in range(b):
            g = [real[env[row]][k] for k in rng.integers(0, 2, h * s)]
            c = np.array([x["pose"][:3] for x in g]) + rng.uniform(-0.5, 0.5, (h * s, 3)) * np.array([x["shape"] for x in g]) * VS * 1.6
            sph[row, ..., :3] = c.reshape(h, s, 3)
            sph[row, ..., 3] = rng.choice([0.02, 0.04], (h, s))
        cases.append(VoxelCase(f"store_{b * h * s}", arrays, sph, 0.02, 2.0, env=env))
    return cases


SLACK_VOXELS = (-1.0, 0.6, 1.0, 2.0, 3.0, 3.4, 3.6, 5.0)


def slack_window():
    """The one place where the sweep cull's slack of 3.5 voxels + 0.2 % of the distance decides a result.  Below a clearance of
    1000 m the cull only skips what the sweep loop would skip itself (its first step is the clearance, which already exceeds
    the half step).  At 1000 m and more the reference steps by r + eta instead, so a culled direction loses samples.  One
    voxel of 2000 in a grid of -0.05 (not 1-Lipschitz), a sphere on that voxel's centre with r + eta = two voxels, neighbours
    4 km away along x: column k's half step leaves  clearance - 1.0001 half_step - 0.002 * 2000 - 1e-6 = SLACK_VOXELS[k] voxels,
    so the kernel must keep sampling in the columns below 3.5 (and finds the occupied voxels two voxels on, like the
    reference) and may cull above.  -> (case with spheres [1, 3, 8, 4], SLACK_VOXELS)"""
    v = np.full((8, 8, 8), -0.05)
    v[2, 4, 4] = 2000.0
    g = make_grid((8, 8, 8), values=v)
    centre = (np.array([2, 4, 4]) + 0.5 - 4.0) * VS
    r, eta = 0.105, 0.02
    k = np.asarray(SLACK_VOXELS)
    half = (2000.0 - (r + eta) - 0.002 * 2000.0 - 1e-6 - k * VS) / 1.0001
    sph = np.zeros((1, 3, len(k), 4))
    sph[..., :3] = centre
    sph[0, 0, :, 0] -= 2 * half
    sph[0, 2, :, 0] += 2 * half
    sph[..., 3] = r
    return VoxelCase("slack_window", stack_voxel_grids([[g]], max_distance=10000.0), sph.astype(np.float32), eta, 1.0, lipschitz=False), k


def family(name):
    """the cases of one family (a list: some families hold several stores or layouts)"""
    rng = np.random.default_rng(FAMILIES.index(name) + 11)
    if name == "thin":
        return [_thin(rng)]
    if name == "shell":
        return [_shell_like("shell", rng, (0, 0, 0, 1, 0, 0, 0), (1.0, 0.5, 0, 1, 0, 0, 0), 0.0)]
    if name == "pose":  # rotated and translated; the lattice 1/16 voxel off the cell boundaries
        return [_shell_like("pose", rng, (0.13, -0.07, 0.21, 0.8, 0.3, -0.4, 0.33), (1.1, 0.4, -0.2, 0.5, -0.6, 0.2, 0.59), 0.0625)]
    if name == "store":
        return _store(rng)
    if name == "truncated":  # 0.125 is exact in fp16 (stored values EQUAL max_distance), fp16(0.1) < 0.1f (they never do)
        return [_truncated(rng, 0.125), _truncated(rng, 0.1)]
    if name == "extremes":
        return [_extremes(rng)]
    if name == "sweep":
        return [_sweep(rng)]
    if name == "coarse":
        return [_coarse(rng)]
    if name == "step":
        return [_step(rng)]
    raise KeyError(name)


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
