"""Golden vectors for sphere-MESH collision, produced by the REFERENCE's own Warp kernels executed on the CPU.

    PYTHONPATH=/root/reference python tests/golden/make_mesh_warp_golden.py

The companion of ``make_scene_warp_golden.py`` (see its docstring): with ``tests/golden/warp_emulator`` on the path as
``warp``, the reference's unmodified sources are imported and run thread by thread in fp32:

    curobo/_src/geom/collision/wp_collision_kernel.py        sphere_obstacle_collision_kernel
    curobo/_src/geom/collision/wp_sweep_collision_kernel.py  swept_sphere_obstacle_collision_kernel (SWEEP_STEPS = 3)
    curobo/_src/geom/collision/wp_speed_metric.py            apply_speed_metric
    curobo/_src/geom/data/data_mesh.py                       MeshDataWarp, compute_local_sdf_with_grad (search range
                                                             max(half bounding-box diagonal, radius_adjusted), the
                                                             (max_distance, 0) answer, the gradient -(closest - p) / |.|),
                                                             WarpMeshCache.get_bounds (the dims of a slot)
    curobo/_src/geom/data/data_cuboid.py                     cuboids of the mixed world

Warp's mesh intrinsics (``wp.Mesh``, ``wp.mesh_query_point`` with the three-ray sign of ``mesh_query_inside``,
``wp.mesh_eval_position``) are restated in the emulator.  The launches follow wp_autograd.py: outputs zeroed once, one launch
per obstacle kind in the order of SceneData.get_valid_data (cuboids, then meshes), the speed metric once afterwards.

Every mesh query the kernels make is recorded and checked here, so that the golden encodes no knife edge:
  * a penetration -sdf + radius_adjusted within 1e-4 of zero (the in-collision flag would turn on rounding),
  * a found distance within 1e-5 of the search range (found / not found would),
  * a second triangle within 2e-6 of the closest one whose closest point lies elsewhere (the gradient would),
  * a ray of the sign test that passes within 1e-6 (barycentric) of an edge or starts within 1e-6 of a face.
Spheres that make such a query are left out of the per-case ``mask`` (True = trusted), those with a tie only out of
``grad_mask``; the counts are printed.  On closed
meshes the three-ray sign must equal the winding-number sign at every found query (asserted).  The output is
tests/golden/mesh_warp_golden.npz: arrays and names only, in the layout of ``curobo_amd.scene.mesh.MeshStore``.
"""
import importlib.abc
import importlib.machinery
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "warp_emulator"))
sys.path.insert(1, TESTS)
sys.path.append(os.path.dirname(TESTS))  # (last: the repository's own curobo/ package must not shadow the reference's)


class _StubMissing(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """third-party modules the reference's geometry types import at module level and these kernels never touch"""

    ROOTS = {"trimesh"}

    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in self.ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = MagicMock(name=spec.name)
        m.__path__, m.__name__, m.__spec__, m.__loader__ = [], spec.name, spec, self
        return m

    def exec_module(self, module):
        pass


sys.meta_path.append(_StubMissing())

import warp as wp  # noqa: E402  (the emulator)

import curobo._src.geom.collision.wp_collision_kernel as K  # noqa: E402
import curobo._src.geom.collision.wp_sweep_collision_kernel as KS  # noqa: E402
from curobo._src.geom.collision.wp_speed_metric import apply_speed_metric  # noqa: E402
from curobo._src.geom.data.data_mesh import MeshDataWarp, WarpMeshCache  # noqa: E402

assert "emulator" in (wp.__doc__ or "") or "stand-in" in (wp.__doc__ or ""), "the real warp is on the path: not this script's case"

from make_scene_warp_golden import cuboid_arrays, cuboid_struct, inverse_pose7  # noqa: E402
from test_oracle_mesh import box_shape, ell_shape, is_closed_and_oriented, sphere_shape, torus_shape  # noqa: E402
from test_oracle_mesh_sign import face_normals, plate, with_flipped, without_faces_facing  # noqa: E402


# ---------------------------------------------------------------- fixtures
def sliver_box(near_zero=False):
    """a closed, consistently oriented box [-.1, .1] x [-.075, .075] x [-.05, .05] whose top face is split along its diagonal
    P0 -> P2 with a T-junction: one side is a single triangle, the other two triangles meeting at M on the diagonal (at 0.3 of
    its length), and the sliver (P0, P2, M) closes the junction -- zero area (M on the diagonal), or near zero (M moved 1e-5
    off it towards P3, the side that keeps the sliver's normal outward)"""
    a, b, c = 0.1, 0.075, 0.05
    v = [[-a, -b, -c], [a, -b, -c], [a, b, -c], [-a, b, -c], [-a, -b, c], [a, -b, c], [a, b, c], [-a, b, c]]
    p0, p2, p3 = np.array(v[4]), np.array(v[6]), np.array(v[7])
    m = p0 + 0.3 * (p2 - p0)
    if near_zero:
        d = p2 - p0
        perp = np.array([-d[1], d[0], 0.0]) / np.linalg.norm(d[:2])
        m = m + 1e-5 * perp * np.sign(np.dot(perp, p3 - p0))
    v.append(list(m))
    M = 8
    f = [[0, 2, 1], [0, 3, 2],                  # bottom (-z)
         [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7],
         [4, 5, 6],                             # top: P0 P1 P2
         [4, M, 7], [M, 6, 7],                  # top: P0 M P3, M P2 P3
         [4, 6, M]]                             # the sliver: edges P0->P2, P2->M, M->P0
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def open_fixtures():
    """tests/test_gpu_mesh.py::_open_fixtures"""
    vb, fb = box_shape([0.3, 0.5, 0.2], 2)
    n = face_normals(vb, fb)
    return [("open_box_pz", *without_faces_facing(vb, fb, [0, 0, 1])), ("open_box_mz", *without_faces_facing(vb, fb, [0, 0, -1])),
            ("single_sided_plate", *plate()), ("box_one_flipped_face", *with_flipped(vb, fb, [np.flatnonzero(n[:, 0] > 0.999)[3]]))]


def rot(ax, ang):
    ax = np.asarray(ax, np.float64)
    return [np.cos(ang / 2), *(np.sin(ang / 2) * ax / np.linalg.norm(ax))]


def quat_rot(q, v):
    w, x, y, z = q
    u = np.array([x, y, z])
    return v * (2 * w * w - 1) + 2 * w * np.cross(u, v) + 2 * u * np.dot(u, v)


# ---------------------------------------------------------------- geometry checks (fp64)
def tri_distances(p, v, f):
    """distance of p to every triangle and the closest point on it (Ericson, fp64)"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    p = np.asarray(p, np.float64)[None]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    dot = lambda x, y: np.einsum("ij,ij->i", x, y)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.select([((d1 <= 0) & (d2 <= 0))[:, None], ((d3 >= 0) & (d4 <= d3))[:, None], ((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None],
                       ((d6 >= 0) & (d5 <= d6))[:, None], ((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None],
                       ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None]],
                      [a, b, a + (d1 / (d1 - d3))[:, None] * ab, c, a + (d2 / (d2 - d6))[:, None] * ac,
                       b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b)],
                      a + (vb / (va + vb + vc))[:, None] * ab + (vc / (va + vb + vc))[:, None] * ac)
    d = np.linalg.norm(p - q, axis=1)
    return np.where(np.isfinite(d), d, np.inf), q


def winding_inside(p, v, f):
    a, b, c = (v[f[:, k]].astype(np.float64) - np.asarray(p, np.float64) for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
    dot = lambda x, y: np.einsum("ij,ij->i", x, y)  # noqa: E731
    num = dot(a, np.cross(b, c))
    den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
    return abs((2 * np.arctan2(num, den)).sum()) > 2 * np.pi


def ray_ambiguous(p, v, f, eps=1e-6):
    """a ray of the three-ray sign test passes within eps (barycentric) of an edge or a vertex of a face it may hit first, or
    the point lies within eps of a face along a ray"""
    vv = v.astype(np.float64)
    a, b, c = vv[f[:, 0]], vv[f[:, 1]], vv[f[:, 2]]
    ab, ac, tv = b - a, c - a, np.asarray(p, np.float64)[None] - a
    for axis in range(3):
        d = np.zeros(3)
        d[axis] = 1.0
        pv = np.cross(d[None], ac)
        det = np.einsum("ij,ij->i", ab, pv)
        live = np.abs(det) > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.einsum("ij,ij->i", tv, pv) / det
            qv = np.cross(tv, ab)
            w = (qv @ d) / det
            t = np.einsum("ij,ij->i", ac, qv) / det
        m = np.minimum(np.minimum(u, w), 1 - u - w)
        hit = live & (m >= 0) & (t > 0)
        t_first = t[hit].min() if hit.any() else np.inf
        near_edge = live & (np.abs(m) < eps) & (t > -eps) & (t <= t_first + eps)
        if near_edge.any() or (live & (m > -eps) & (np.abs(t) < eps)).any():
            return True
    return False


# ---------------------------------------------------------------- worlds
def mesh_slots(envs, max_n):
    """envs[e] = list of {"mesh": key, "pose", "enable"}; -> MeshStore-layout arrays + the emulator's meshes"""
    E = len(envs)
    mesh_id, dims = np.zeros((E, max_n), np.int32), np.zeros((E, max_n, 4), np.float32)
    inv_pose, pose = np.zeros((E, max_n, 8), np.float32), np.zeros((E, max_n, 7), np.float32)
    inv_pose[..., 3], pose[..., 3] = 1.0, 1.0
    enable, count = np.zeros((E, max_n), np.uint8), np.zeros((E,), np.int32)
    for e, obs in enumerate(envs):
        count[e] = len(obs)
        for i, o in enumerate(obs):
            mesh_id[e, i] = o["mesh"]
            pose[e, i] = o["pose"]
            inv_pose[e, i, :7] = inverse_pose7(o["pose"])
            enable[e, i] = 1 if o.get("enable", True) else 0
    return {"mesh_id": mesh_id, "dims": dims, "inv_pose": inv_pose, "pose": pose, "enable": enable, "count": count}


class World:
    def __init__(self, name, meshes, envs, max_n, cuboids=None):
        self.name, self.meshes = name, meshes  # meshes: list of (name, vertices, faces)
        self.slots = mesh_slots(envs, max_n)
        self.cuboids = cuboids
        self.wp_meshes, caches = [], []
        for mname, v, f in meshes:
            m = wp.Mesh(points=wp.array(v, dtype=wp.vec3), indices=wp.array(np.ravel(f).astype(np.int32), dtype=wp.int32))
            self.wp_meshes.append(m)
            caches.append(WarpMeshCache(mname, m.id, m.points, m.indices, m))
        self.closed = np.array([is_closed_and_oriented(f) for _n, _v, f in meshes])
        for e in range(len(envs)):
            for i in range(int(self.slots["count"][e])):
                lo, hi = caches[self.slots["mesh_id"][e, i]].get_bounds()  # the reference's dims (data_mesh.py, load_batch / add)
                self.slots["dims"][e, i, :3] = (hi - lo).numpy()

    def struct(self):
        s = self.slots
        E, n = s["mesh_id"].shape
        ids = np.array([int(self.wp_meshes[k].id) for k in s["mesh_id"].reshape(-1)], np.uint64)
        return MeshDataWarp(mesh_ids=wp.array(ids, dtype=wp.uint64), dims=wp.array(s["dims"].reshape(E * n, 4), dtype=wp.float32),
                            inv_pose=wp.array(s["inv_pose"].reshape(E * n, 8), dtype=wp.float32),
                            enable=wp.array(s["enable"].reshape(-1), dtype=wp.uint8), n_per_env=wp.array(s["count"], dtype=wp.int32),
                            max_n=wp.int32(n), num_envs=wp.int32(E), max_dist=wp.float32(0.1))

    def surface_points(self, rng, n, env=0):
        """world-frame points on the enabled meshes of env, with the outward (face) normal"""
        s = self.slots
        live = [i for i in range(int(s["count"][env])) if s["enable"][env, i]]
        out, nrm = [], []
        for _ in range(n):
            i = live[rng.integers(len(live))]
            _nm, v, f = self.meshes[s["mesh_id"][env, i]]
            t = f[rng.integers(len(f))]
            w = rng.dirichlet([2.0, 2.0, 2.0])
            q = w @ v[t].astype(np.float64)
            nn = np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]).astype(np.float64)
            nn /= max(np.linalg.norm(nn), 1e-12)
            p7 = s["pose"][env, i].astype(np.float64)
            q7 = p7[3:] / np.linalg.norm(p7[3:])
            out.append(quat_rot(q7, q) + p7[:3])
            nrm.append(quat_rot(q7, nn))
        return np.array(out), np.array(nrm)


# ---------------------------------------------------------------- the reference's launches, with every mesh query recorded
LOG = []


def _recording(fn):
    def rec(obs_set, env_idx, local_idx, local_pt, query_distance):
        r = fn(obs_set, env_idx, local_idx, local_pt, query_distance)
        if isinstance(obs_set, MeshDataWarp):
            LOG.append((int(wp._tid[0]), int(env_idx), int(local_idx), np.array(local_pt.v, np.float32), np.float32(query_distance),
                        np.array(r.v, np.float32)))
        return r

    return rec


K.compute_local_sdf_with_grad = _recording(K.compute_local_sdf_with_grad)
KS.compute_local_sdf_with_grad = _recording(KS.compute_local_sdf_with_grad)


def run(world, spheres, weight, eta, env_idx, multi_env, swept, speed_dt):
    B, H, S, _ = spheres.shape
    n = B * H * S
    dist, grad = np.zeros(n, np.float32), np.zeros(n * 4, np.float32)
    sp = wp.array(spheres.reshape(n, 4).copy(), dtype=wp.vec4)
    kern = KS.swept_sphere_obstacle_collision_kernel if swept else K.sphere_obstacle_collision_kernel
    sets = []
    if world.cuboids is not None:
        sets.append((cuboid_struct(world.cuboids), world.cuboids["cuboid_dims"].shape[1]))
    sets.append((world.struct(), world.slots["mesh_id"].shape[1]))
    LOG.clear()
    for obs, max_n in sets:
        wp.launch(kern, dim=n * max_n,
                  inputs=[obs, sp, wp.array(np.array([weight], np.float32)), wp.array(np.array([eta], np.float32)),
                          wp.array(np.asarray(env_idx, np.int32))],
                  outputs=[wp.array(dist), wp.array(grad), wp.int32(B), wp.int32(H), wp.int32(S), wp.int32(max_n),
                           wp.uint8(1 if multi_env else 0)])
    if speed_dt is not None:
        wp.launch(apply_speed_metric, dim=n,
                  inputs=[sp, wp.array(dist), wp.array(grad), wp.array(np.array([speed_dt], np.float32)), wp.int32(B), wp.int32(H),
                          wp.int32(S)])
    return dist.reshape(B, H, S), grad.reshape(B, H, S, 4), list(LOG)


def review(world, log, n_spheres):
    """per sphere: trusted (no knife edge), the mesh slots it collided with (bits), the side of its colliding queries (+1 all
    outside, -1 all inside, 0 mixed / none), the smallest |sdf| among them; and the branch counts of the case"""
    max_n = world.slots["mesh_id"].shape[1]
    trusted = np.ones(n_spheres, bool)
    tied = np.zeros(n_spheres, bool)  # (a tie leaves the distance well defined: only the gradient is left out)
    slots_hit = np.zeros(n_spheres, np.int32)
    side = np.zeros((n_spheres, 2), np.int32)  # colliding queries outside / inside
    near = np.full(n_spheres, np.inf, np.float32)  # the smallest |sdf| of a colliding query
    st = dict(queries=0, found=0, not_found=0, inside=0, outside=0, beyond_half_diag=0, knife=0, tie=0, ray=0)
    for tid, env, slot, lp, qd, r in log:
        sph = tid // max_n
        st["queries"] += 1
        half = np.float32(np.float32(0.5) * np.float32(np.sqrt(np.float32(np.sum(world.slots["dims"][env, slot, :3].astype(np.float32) ** 2)))))
        max_d = max(half, qd)
        _nm, v, f = world.meshes[world.slots["mesh_id"][env, slot]]
        found = not (r[0] == max_d and not r[1:].any())
        pen = -r[0] + qd
        # (nothing found: pen = radius_adjusted - max(half diagonal, radius_adjusted) <= 0, exactly 0 in the query_distance
        # branch -- the same fp32 operations on every path, no knife edge)
        bad = found and abs(pen) < 1e-4
        st["knife"] += int(bad)
        if pen > 0:
            slots_hit[sph] |= 1 << slot
            near[sph] = min(near[sph], abs(r[0]))
            side[sph, 0 if r[0] > 0 else 1] += 1
        if found:
            st["found"] += 1
            st["inside" if r[0] < 0 else "outside"] += 1
            st["beyond_half_diag"] += int(abs(r[0]) >= half)
            d, q = tri_distances(lp, v, f)
            k = int(np.argmin(d))
            bad |= abs(d[k] - max_d) < 1e-5
            # another triangle about as close whose closest point is elsewhere (not the shared edge / vertex): the direction
            # of the gradient would turn on rounding
            other = np.linalg.norm(q - q[k], axis=1) > 1e-6
            if other.any() and d[other].min() - d[k] < 2e-6:
                st["tie"] += 1
                tied[sph] = True
            if ray_ambiguous(lp, v, f):
                st["ray"] += 1
                bad = True
            elif world.closed[world.slots["mesh_id"][env, slot]] and d[k] > 1e-6:
                assert (r[0] < 0) == winding_inside(lp, v, f), (world.name, lp, r)
        else:
            st["not_found"] += 1
            bad |= tri_distances(lp, v, f)[0].min() - max_d < 1e-5
        if bad:
            trusted[sph] = False
    sign = np.where((side[:, 0] > 0) & (side[:, 1] == 0), 1, np.where((side[:, 1] > 0) & (side[:, 0] == 0), -1, 0)).astype(np.int8)
    return trusted, tied, slots_hit, sign, near, st


# ---------------------------------------------------------------- spheres
def spheres_near(world, rng, B, H, S, radii, step, offset=(-0.06, 0.08), env_of_b=None):
    """trajectories that start near the surfaces of the meshes of the batch's environment and drift"""
    sp = np.zeros((B, H, S, 4), np.float32)
    for b in range(B):
        env = 0 if env_of_b is None else int(env_of_b[b])
        p, n = world.surface_points(rng, S, env)
        start = p + n * rng.uniform(*offset, size=(S, 1))
        drift = step * rng.uniform(-1, 1, (1, S, 3)) * np.arange(H).reshape(H, 1, 1)
        sp[b, :, :, :3] = start[None] + drift + 0.1 * step * rng.standard_normal((H, S, 3))
        sp[b, :, :, 3] = rng.choice(radii, (1, S))
    return sp


def main():
    rng = np.random.default_rng(20261016)
    # closed meshes (tests/test_oracle_mesh.py), small enough for a brute-force query per thread
    closed = [("box", *box_shape([0.3, 0.4, 0.2], 1)), ("ball", *sphere_shape(0.12, 10, 20)), ("torus", *torus_shape(0.15, 0.05, 24, 12)),
              ("ell", *ell_shape(1)), ("tiny", *box_shape([0.04, 0.04, 0.04], 0))]
    env0 = [{"mesh": 0, "pose": [0.5, 0.0, 0.3, *rot([0, 0, 1], 0.5)]},
            {"mesh": 1, "pose": [0.2, 0.4, 0.5, *rot([1, 1, 0], 0.8)]},
            {"mesh": 2, "pose": [0.2, -0.4, 0.5, *rot([1, 0, 0], 1.1)]},
            {"mesh": 3, "pose": [-0.3, 0.1, 0.2, *rot([0.3, -0.5, 0.8], 1.7)]},
            {"mesh": 4, "pose": [0.0, 0.0, 0.8, *rot([0, 1, 0], 0.3)]},
            {"mesh": 1, "pose": [-0.2, -0.2, 0.7, 1, 0, 0, 0], "enable": False}]
    env1 = [{"mesh": 3, "pose": [0.4, 0.3, 0.3, *rot([0, 0, 1], -0.9)]},
            {"mesh": 0, "pose": [-0.1, -0.3, 0.4, *rot([1, 2, 0], -0.5)]},
            {"mesh": 4, "pose": [0.3, -0.1, 0.6, 1, 0, 0, 0]}]
    w_closed = World("closed", closed, [env0, env1], max_n=7)
    w_mixed = World("mixed", closed[:3], [env0[:3]], max_n=3,
                    cuboids=cuboid_arrays([[{"dims": [0.3, 0.3, 0.05], "pose": [0.45, 0.05, 0.42, *rot([0, 0, 1], 0.2)]},
                                            {"dims": [0.1, 0.2, 0.3], "pose": [0.2, 0.3, 0.45, *rot([1, 0, 0], 0.4)]}]], max_n=2))
    opens = open_fixtures()
    w_open = World("open", opens, [[{"mesh": k, "pose": p} for k, p in enumerate(
        [[0.0, 0.0, 0.3, *rot([0, 1, 0], 0.5)], [0.8, 0.0, 0.3, *rot([1, 0, 0], -0.4)], [0.0, 0.8, 0.3, *rot([1, 1, 0], 0.3)],
         [0.8, 0.8, 0.3, *rot([0, 0, 1], 0.7)]])]], max_n=4)
    slivers = [("sliver_zero_area", *sliver_box(False)), ("sliver_near_zero_area", *sliver_box(True))]
    w_sliver = World("sliver", slivers, [[{"mesh": 0, "pose": [0.3, 0.0, 0.4, *rot([1, 2, 3], 0.6)]},
                                          {"mesh": 1, "pose": [-0.3, 0.2, 0.4, *rot([-2, 1, 1], 1.2)]}]], max_n=2)
    for _nm, _v, f in closed + slivers:
        assert is_closed_and_oriented(f), _nm

    radii = np.array([0.01, 0.025, 0.04, 0.06, -1.0], np.float32)  # a negative radius disables a sphere
    out, worlds, meta = {}, {}, []

    def add_world(w, sp, env_idx):
        worlds[w.name] = w
        for k, v in w.slots.items():
            out[f"{w.name}/{k}"] = v
        for i, (mname, v, f) in enumerate(w.meshes):
            out[f"{w.name}/mesh{i}/vertices"], out[f"{w.name}/mesh{i}/faces"] = v.astype(np.float32), f.astype(np.int32)
        out[f"{w.name}/mesh_names"] = np.array([m[0] for m in w.meshes])
        out[f"{w.name}/closed"] = w.closed
        if w.cuboids is not None:
            for k, v in w.cuboids.items():
                out[f"{w.name}/{k}"] = v
        out[f"{w.name}/spheres"], out[f"{w.name}/env_query_idx"] = sp, env_idx

    # closed: two environments, special spheres
    B, H, S = 4, 5, 12
    env_idx = np.array([0, 1, 0, 1], np.int32)
    sp = spheres_near(w_closed, rng, B, H, S, radii, 0.012, env_of_b=env_idx)
    sp[0, :, 0] = [3.0, 3.0, 3.0, 0.05]                 # far outside everything: nothing found
    # deep inside the box and near the ball's centre (off the exact centres, where opposite faces tie)
    sp[2, :, 1, :3] = quat_rot(np.asarray(env0[0]["pose"][3:]), np.array([0.02, -0.03, 0.011])) + env0[0]["pose"][:3]
    sp[2, :, 2, :3] = np.array([0.2, 0.4, 0.5]) + [0.021, -0.013, 0.017]
    sp[2, :, 1:3, 3] = 0.03
    sp[2, :, 3] = [0.0, 0.0, 0.8 + 0.07, 0.06]          # above the tiny box: its half diagonal (0.035) < radius_adjusted
    sp[0, :, 4] = [0.0, 0.06, 0.8, 0.05]                # beside it
    sp[2, :, 5, 3] = -1.0
    sp[1, :, 0, :3] = sp[1, 0:1, 0, :3]                 # stationary (the sweep loops do not run)
    add_world(w_closed, sp, env_idx)
    # mixed cuboids + meshes, one environment
    sp = spheres_near(w_mixed, rng, 3, 5, 12, radii, 0.01)
    add_world(w_mixed, sp, np.zeros(3, np.int32))
    # open and flipped meshes
    sp = spheres_near(w_open, rng, 3, 5, 12, radii, 0.01, offset=(-0.05, 0.06))
    add_world(w_open, sp, np.zeros(3, np.int32))
    # slivers: centres just inside the top face, next to the diagonal that carries the sliver, on both sides of it
    sp = np.zeros((2, 4, 16, 4), np.float32)
    for b in range(2):
        mname, v, f = slivers[b]
        p7 = np.asarray(w_sliver.slots["pose"][0, b], np.float64)
        q7 = p7[3:] / np.linalg.norm(p7[3:])
        p0, p2 = v[4].astype(np.float64), v[6].astype(np.float64)
        d = p2 - p0
        perp = np.array([-d[1], d[0], 0.0]) / np.linalg.norm(d[:2])
        for s_ in range(16):
            t = rng.uniform(0.08, 0.92) if s_ % 4 else 0.3 + rng.uniform(-0.01, 0.01)  # (every fourth next to M)
            off = rng.choice([-1, 1]) * rng.uniform(2e-4, 4e-3)
            depth = rng.uniform(3e-3, 2e-2)
            base = p0 + t * d + off * perp - np.array([0, 0, depth])
            for h in range(4):
                lp = base + np.array([0, 0, -0.004 * h]) + 1e-3 * h * perp * (1 if s_ % 2 else -1)
                sp[b, h, s_, :3] = quat_rot(q7, lp) + p7[:3]
        sp[b, :, :, 3] = rng.choice([0.01, 0.02, 0.03], (1, 16))
    add_world(w_sliver, sp, np.zeros(2, np.int32))

    cases = [  # name, world, weight, eta, multi_env, swept, speed_dt
        ("closed_static", "closed", 1.0, 0.02, True, False, None),
        ("closed_static_eta0", "closed", 2.5, 0.0, True, False, None),
        ("closed_swept", "closed", 1.0, 0.02, True, True, None),
        ("closed_swept_speed", "closed", 5.0, 0.02, True, True, 0.05),
        ("closed_static_speed", "closed", 1.0, 0.02, True, False, 0.02),
        ("closed_env0_only", "closed", 1.0, 0.02, False, False, None),
        ("mixed_static", "mixed", 1.0, 0.02, False, False, None),
        ("mixed_swept_speed", "mixed", 3.0, 0.025, False, True, 0.05),
        ("open_static", "open", 1.0, 0.02, False, False, None),
        ("open_swept", "open", 2.0, 0.02, False, True, None),
        ("sliver_static", "sliver", 1.0, 0.02, False, False, None),
        ("sliver_swept", "sliver", 1.0, 0.02, False, True, None),
    ]
    for name, wname, wgt, eta, multi, swept, dt in cases:
        w = worlds[wname]
        sph, env = out[f"{wname}/spheres"], out[f"{wname}/env_query_idx"]
        d, g, log = run(w, sph, wgt, eta, env, multi, swept, dt)
        trusted, tied, slots_hit, sign, near, st = review(w, log, d.size)
        out[f"{name}/distance"], out[f"{name}/gradient"] = d, g
        out[f"{name}/mask"] = trusted.reshape(d.shape)
        out[f"{name}/grad_mask"] = (trusted & ~tied).reshape(d.shape)
        out[f"{name}/slots_hit"], out[f"{name}/side"] = slots_hit.reshape(d.shape), sign.reshape(d.shape)
        out[f"{name}/near"] = near.reshape(d.shape)  # (the gradient's direction carries the closest point's rounding / this)
        out[f"{name}/stats"] = np.array([st[k] for k in STATS], np.int64)
        meta.append((name, wname, wgt, eta, int(multi), int(swept), -1.0 if dt is None else dt))
        print(f"{name:20s} hits {int((d > 0).sum()):4d} / {d.size}  masked {int((~trusted).sum()):3d} (+ gradient {int((trusted & tied).sum()):3d})  " +
              " ".join(f"{k} {st[k]}" for k in STATS))
    out["stats_names"] = np.array(STATS)
    out["case_names"] = np.array([m[0] for m in meta])
    out["case_world"] = np.array([m[1] for m in meta])
    out["case_params"] = np.array([m[2:] for m in meta], np.float64)  # weight, eta, multi_env, swept, speed_dt (-1 = off)
    path = os.path.join(HERE, "mesh_warp_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


STATS = ["queries", "found", "not_found", "inside", "outside", "beyond_half_diag", "knife", "tie", "ray"]

if __name__ == "__main__":
    main()
