"""Golden vectors for the mesh-SDF pose refinement (csrc/pose_detect.hip, curobo_amd/perception/pose_estimation), produced by
the REFERENCE's own code on the CPU:

    PYTHONPATH=/root/reference python tests/golden/make_pose_detector_golden.py

evaluation  perception/pose_estimation/wp_mesh_sdf_alignment.py: ``mesh_surface_distance_query_kernel`` and
            ``jacobian_reduce_kernel``, unmodified, thread by thread through tests/golden/warp_emulator (see
            make_scene_warp_golden.py).  Three intrinsics the emulator lacks are defined HERE and set on the ``warp`` module
            before the reference's module is imported: ``mesh_query_point_no_sign`` (``mesh_query_point`` without the sign),
            ``tile`` (a one-element tile per thread) and ``tile_atomic_add``.  Threads run one after the other -- a legal
            schedule -- so the sums come out in thread order.
LM          ``SDFPoseDetector._setup_refinement`` / ``_refine_iteration`` themselves (sdf_pose_detector.py) on CPU tensors with
            ``use_cuda_graph=False``: the reference's ``solve_lm_step``, ``compute_predicted_reduction``, ``trust_region_update``
            (optim_pose_lm.py), ``Pose.from_euler_xyz`` and ``Pose.multiply``, in its own order.  The three functions are wrapped
            only to RECORD their arguments and results.

Cases: see EVAL_CASES / the sequences below.  Output: tests/golden/pose_detector_golden.npz -- arrays, case names and the cfg
defaults only."""
import dataclasses
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reference_robot_loader as _R  # noqa: E402,F401  (the Warp stand-in, the stubs, DeviceCfg held to the CPU)
import torch  # noqa: E402
import warp as wp  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import pose_detector_ref as ORACLE  # noqa: E402  (tests/pose_detector_ref.py: only its excluded set is used here, to place points)


# ------------------------------------------------------------------------------- the three intrinsics the emulator lacks
def mesh_query_point_no_sign(id, point, max_dist):  # noqa: A002
    return wp.mesh_query_point(id, point, max_dist)  # (the callers never read .sign)


def tile(x):
    return wp.Tile(np.array([x], dtype=np.float32))


def tile_atomic_add(arr, t, offset, *a):
    s = arr.a
    s[int(offset)] = s.dtype.type(s[int(offset)] + s.dtype.type(t.a.reshape(-1)[0]))


wp.mesh_query_point_no_sign, wp.tile, wp.tile_atomic_add = mesh_query_point_no_sign, tile, tile_atomic_add

# what sdf_pose_detector.py imports and a CPU run never needs
for _name in ("curobo._src.curobolib.cuda_ops.tensor_checks",):
    try:
        __import__(_name)
    except Exception:  # noqa: BLE001
        _m = types.ModuleType(_name)
        _m.check_float32_tensors = lambda *a, **k: None
        sys.modules[_name] = _m

import curobo._src.perception.pose_estimation.sdf_pose_detector as SD  # noqa: E402
from curobo._src.perception.pose_estimation.sdf_pose_detector_cfg import SDFDetectorCfg  # noqa: E402
from curobo._src.perception.pose_estimation.wp_mesh_sdf_alignment import (  # noqa: E402
    jacobian_reduce_kernel, mesh_surface_distance_query_kernel)
from curobo._src.types.pose import Pose  # noqa: E402

SD.get_warp_device_stream = lambda t: (None, None)
SD.check_float32_tensors = lambda *a, **k: None


# ----------------------------------------------------------------------------------------------------------- meshes
def strip(n, rng):
    """n triangles: a zig-zag strip with a gentle twist (open)"""
    k = n + 2
    i = np.arange(k)
    v = np.stack([0.04 * (i // 2) + 0.01 * (i % 2), 0.08 * (i % 2) - 0.04, 0.01 * np.sin(0.9 * i)], 1) + rng.normal(0, 0.002, (k, 3))
    f = np.array([[j, j + 1, j + 2] if j % 2 == 0 else [j + 1, j, j + 2] for j in range(n)])
    return v.astype(np.float32), f.astype(np.int32)


def l_solid():
    """an L-shaped prism with a notch: 8-gon extruded, 28 triangles, closed, no symmetry"""
    poly = np.array([[0, 0], [0.16, 0], [0.16, 0.05], [0.09, 0.05], [0.09, 0.08], [0.06, 0.08], [0.06, 0.13], [0, 0.13]], np.float64)
    h = 0.07
    n = len(poly)
    v = np.concatenate([np.c_[poly, np.zeros(n)], np.c_[poly, np.full(n, h)]]) - [0.07, 0.055, 0.03]
    cap = [[0, 1, 2], [0, 2, 3], [0, 3, 5], [3, 4, 5], [0, 5, 6], [0, 6, 7]]  # ear fan that stays inside the polygon
    f = [[a, c, b] for a, b, c in cap] + [[a + n, b + n, c + n] for a, b, c in cap]
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, j + n], [i, j + n, i + n]]
    return v.astype(np.float32), np.array(f, np.int32)


def icosphere(radius=0.08, levels=2):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def sheet():
    """an open wavy sheet, 4 x 3 quads = 24 triangles"""
    x, y = np.meshgrid(np.linspace(-0.1, 0.1, 5), np.linspace(-0.06, 0.06, 4), indexing="ij")
    v = np.stack([x, y, 0.02 * np.sin(18 * x) * np.cos(14 * y)], -1).reshape(-1, 3)
    f = []
    for i in range(4):
        for j in range(3):
            a = i * 4 + j
            f += [[a, a + 4, a + 5], [a, a + 5, a + 1]]
    return v.astype(np.float32), np.array(f, np.int32)


def plane():
    v = np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def quat_from_euler(e):
    return Pose.from_euler_xyz(torch.as_tensor(e, dtype=torch.float32)).quaternion[0].numpy().astype(np.float32)


IDENTITY = (np.zeros(3, np.float32), np.array([1, 0, 0, 0], np.float32))
GENERAL = (np.array([0.31, -0.12, 0.45], np.float32), quat_from_euler([0.4, -0.7, 1.1]))


def to_world(pm, pose):
    p = Pose(position=torch.as_tensor(pose[0])[None], quaternion=torch.as_tensor(pose[1])[None])
    R = p.get_rotation()[0].numpy().astype(np.float64)
    return (pm.astype(np.float64) @ R.T + pose[0].astype(np.float64)).astype(np.float32)


def surface_samples(v, f, n, rng):
    k = rng.integers(0, len(f), n)
    u, w = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = u + w > 1
    u[flip], w[flip] = 1 - u[flip], 1 - w[flip]
    a, b, c = v[f[k, 0]].astype(np.float64), v[f[k, 1]].astype(np.float64), v[f[k, 2]].astype(np.float64)
    nrm = np.cross(b - a, c - a)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    return a + u[:, None] * (b - a) + w[:, None] * (c - a), nrm


def cloud(v, f, n, rng, threshold, far_block=0, near=None):
    """mesh-frame points from 1 mm out to beyond the threshold (log-uniform offsets along the face normal of a surface sample,
    either side for open meshes), ``far_block`` of them well beyond the threshold; ``near``: only that many within it"""
    s, nrm = surface_samples(v, f, n, rng)
    off = np.exp(rng.uniform(np.log(1e-3), np.log(1.6 * threshold), n))
    if near is not None:
        off = np.where(np.arange(n) < near, rng.uniform(0.2, 0.6, n) * threshold, rng.uniform(3.0, 5.0, n) * threshold)
    if far_block:
        off[-far_block:] = rng.uniform(2.5, 4.0, far_block) * threshold
    pm = s + off[:, None] * nrm
    # "far" points leave radially: beyond every face, whatever the concavities
    far = off > 2.0 * threshold
    c = v.astype(np.float64).mean(0)
    d = pm - c
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    reach = np.linalg.norm(v.astype(np.float64) - c, axis=1).max()
    pm[far] = (c + d * (reach + off)[:, None])[far]
    return pm.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- evaluation
def reference_evaluate(points, pose, v, f, threshold, use_huber, delta):
    n = len(points)
    mesh = wp.Mesh(points=wp.array(v, dtype=wp.vec3), indices=wp.array(f.reshape(-1), dtype=wp.int32))
    dist, grad, valid = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    pts = wp.array(np.ascontiguousarray(points), dtype=wp.vec3)
    wp.launch(kernel=mesh_surface_distance_query_kernel, dim=n,
              inputs=[pts, n, wp.array(pose[0]), wp.array(pose[1]), mesh.id, float(threshold), float(threshold), wp.array(dist),
                      wp.array(grad, dtype=wp.vec3), wp.array(valid)])
    JtJ, Jtr, ssq, cnt = np.zeros(36, np.float32), np.zeros(6, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    wp.launch(kernel=jacobian_reduce_kernel, dim=n,
              inputs=[pts, wp.array(dist), wp.array(grad, dtype=wp.vec3), wp.array(valid), n, 1 if use_huber else 0, float(delta),
                      wp.array(JtJ), wp.array(Jtr), wp.array(ssq), wp.array(cnt)])
    return dict(dist=dist, grad=grad, valid=valid, JtJ=JtJ.reshape(6, 6), Jtr=Jtr, sum_sq=ssq, n=cnt)


MESHES = {"tri1": lambda r: strip(1, r), "tri7": lambda r: strip(7, r), "tri8": lambda r: strip(8, r), "tri9": lambda r: strip(9, r),
          "tri12": lambda r: strip(12, r), "lsolid": lambda r: l_solid(), "ico320": lambda r: icosphere(), "sheet": lambda r: sheet(),
          "plane": lambda r: plane()}
# name: mesh, pose, N, threshold, huber (None: off), extras
EVAL_CASES = [
    ("tri1_n1", "tri1", IDENTITY, 1, 0.05, None, {}),
    ("tri7_n63", "tri7", GENERAL, 63, 0.05, 0.02, {}),
    ("tri8_n64", "tri8", IDENTITY, 64, 0.05, None, {}),
    ("tri9_n65", "tri9", GENERAL, 65, 0.05, 0.02, {}),
    ("tri12_n255", "tri12", GENERAL, 255, 0.08, 0.03, {}),
    ("lsolid_n256", "lsolid", IDENTITY, 256, 0.05, None, {}),
    ("lsolid_n257", "lsolid", GENERAL, 257, 0.05, 0.02, {"far_block": 40}),
    ("ico_n1023", "ico320", GENERAL, 1023, 0.05, 0.02, {"awkward": True}),
    ("lsolid_n1023_id", "lsolid", IDENTITY, 1023, 0.06, 0.02, {"awkward": True, "far_block": 100}),
    ("sheet_n1023", "sheet", GENERAL, 1023, 0.05, None, {"awkward": True}),
    ("ico_n5003", "ico320", GENERAL, 5003, 0.2, 0.1, {"far_block": 300}),
    ("lsolid_zero_valid", "lsolid", GENERAL, 65, 0.02, 0.01, {"near": 0}),
    ("lsolid_valid10", "lsolid", GENERAL, 63, 0.05, 0.02, {"near": 10}),
    ("lsolid_valid11", "lsolid", GENERAL, 64, 0.05, 0.02, {"near": 11}),
    ("plane_singular", "plane", IDENTITY, 255, 0.2, None, {"plane": True}),
]


def awkward_points(v, f):
    """exactly on a vertex, on an edge midpoint and on a face centroid (mesh frame): dist <= 1e-8, invalid"""
    a, b, c = v[f[0, 0]], v[f[0, 1]], v[f[0, 2]]
    return np.stack([a, (0.5 * (a.astype(np.float64) + b)).astype(np.float32), ((a.astype(np.float64) + b + c) / 3).astype(np.float32)])


def eval_cases(out):
    rng = np.random.default_rng(4242)
    names = []
    for name, mesh, pose, n, thr, huber, extra in EVAL_CASES:
        v, f = MESHES[mesh](rng)
        if extra.get("plane"):  # all points over one side of the plane: J^T J has rank 3
            gen = lambda k: np.c_[rng.uniform(-0.15, 0.15, (k, 2)), rng.uniform(0.002, 0.1, k)].astype(np.float32)  # noqa: E731
        else:
            gen = lambda k: cloud(v, f, k, rng, thr)  # noqa: E731
        pm = gen(n) if "near" not in extra and not extra.get("far_block") else cloud(v, f, n, rng, thr, extra.get("far_block", 0), extra.get("near"))
        # the fixture keeps the oracle's excluded set (tests/pose_detector_ref.py) to the points put there on purpose: a point
        # the oracle would exclude (e.g. over the diagonal of a flat face: two closest points 10 um apart at one distance) is drawn again
        for _ in range(50):
            ex = ORACLE.evaluate(pm, IDENTITY[0], IDENTITY[1], v, f, thr, thr, False, 0.0)["excluded"]
            if not ex.any():
                break
            assert "near" not in extra or not ex[: extra["near"]].any(), name
            fresh = gen(int(ex.sum()))
            if "near" in extra or extra.get("far_block"):  # (far points stay far: only their direction is drawn again)
                d = fresh - v.mean(0)
                fresh = (v.mean(0) + d / np.linalg.norm(d, axis=1, keepdims=True) * np.linalg.norm(pm[ex] - v.mean(0), axis=1, keepdims=True)).astype(np.float32)
                keep_class = ORACLE.evaluate(pm[ex], IDENTITY[0], IDENTITY[1], v, f, thr, thr, False, 0.0)["raw_dist"] > 1.5 * thr
                fresh = np.where(keep_class[:, None], fresh, gen(int(ex.sum())))
            pm[ex] = fresh
        if extra.get("awkward"):
            pm[:3] = awkward_points(v, f)
        pts = to_world(pm, pose)
        r = reference_evaluate(pts, pose, v, f, thr, huber is not None, huber or 0.0)
        out.update({f"{name}/vertices": v, f"{name}/faces": f, f"{name}/points": pts, f"{name}/position": pose[0], f"{name}/quaternion": pose[1],
                    f"{name}/params": np.array([thr, thr, 0.0 if huber is None else 1.0, huber or 0.0], np.float64)})
        out.update({f"{name}/{k}": val for k, val in r.items()})
        names.append(name)
        print(name, "N", n, "triangles", len(f), "valid", int(r["n"][0]), "sum_sq", float(r["sum_sq"][0]))
        if "near" in extra:
            assert int(r["n"][0]) == extra["near"], (name, int(r["n"][0]))
    out["eval_case_names"] = np.array(names)


# ----------------------------------------------------------------------------------------------------------- LM sequences
class _Rigid:
    """what SDFPoseDetector reads of a RobotMesh"""

    def __init__(self, v, f):
        self.device = "cpu"
        self._mesh = wp.Mesh(points=wp.array(v, dtype=wp.vec3), indices=wp.array(f.reshape(-1), dtype=wp.int32))
        self.mesh_id = self._mesh.id


STATE_KEYS = ("best_position", "best_quaternion", "best_error", "best_sum_sq", "best_n_valid", "best_JtJ", "best_Jtr", "lambda_damping")


def snapshot(state):
    return {k: np.array(getattr(state, k).detach().numpy(), copy=True).reshape(-1) for k in STATE_KEYS}


def run_sequence(out, name, v, f, points, init_pose, truth, cfg, n_iter):
    rec = {}
    real = (SD.solve_lm_step, SD.compute_predicted_reduction, SD.trust_region_update)

    def solve(JtJ, Jtr, lam, eye):
        d = real[0](JtJ, Jtr, lam, eye)
        rec["delta"] = d.detach().numpy().copy()
        return d

    def pred(delta, Jtr, JtJ):
        p = real[1](delta, Jtr, JtJ)
        rec["pred"] = np.float32(p.item())
        return p

    def trust(**kw):
        res = real[2](**kw)
        rec.update(cand_position=kw["cand_position"].numpy().copy(), cand_quaternion=kw["cand_quaternion"].numpy().copy(),
                   cand_JtJ=kw["cand_JtJ"].numpy().copy().reshape(-1), cand_Jtr=kw["cand_Jtr"].numpy().copy(),
                   cand_sum_sq=np.float32(kw["sum_sq_residuals"].item()), cand_n_valid=np.int32(kw["cand_n_valid"].item()))
        lam, new = np.float32(kw["lambda_damping"].item()), np.float32(res[7].item())
        down = np.float32(min(max(lam / np.float32(kw["lambda_factor"]), np.float32(kw["lambda_min"])), np.float32(kw["lambda_max"])))
        rec["accepted"] = np.int32(new == down)
        return res

    SD.solve_lm_step, SD.compute_predicted_reduction, SD.trust_region_update = solve, pred, trust
    try:
        det = SD.SDFPoseDetector(_Rigid(v, f), cfg)
        pose = Pose(position=torch.as_tensor(init_pose[0])[None].clone(), quaternion=torch.as_tensor(init_pose[1])[None].clone())
        state = det._setup_refinement(torch.as_tensor(points), pose).clone()
        rows = []
        for it in range(n_iter):
            before = snapshot(state)
            state = det._refine_iteration(state).clone()
            row = {f"before_{k}": val for k, val in before.items()}
            row.update(rec)
            row.update({f"after_{k}": val for k, val in snapshot(state).items()})
            rows.append(row)
            print(f"  {name} it {it:2d} accepted {int(rec['accepted'])} lambda {float(before['lambda_damping'][0]):.1e} n {int(rec['cand_n_valid'])} "
                  f"error {float(snapshot(state)['best_error'][0]):.3e}")
    finally:
        SD.solve_lm_step, SD.compute_predicted_reduction, SD.trust_region_update = real
    for k in rows[0]:
        out[f"{name}/{k}"] = np.stack([np.asarray(r[k]) for r in rows])
    fp, fq = rows[-1]["after_best_position"].astype(np.float64), rows[-1]["after_best_quaternion"].astype(np.float64)
    t_err = float(np.linalg.norm(fp - truth[0]))
    qt = truth[1].astype(np.float64)
    w = fq @ qt  # the relative rotation qt^-1 fq: angle = 2 atan2(|vector part|, |w|) (accurate near 0, unlike arccos)
    vec = qt[0] * fq[1:] - fq[0] * qt[1:] - np.cross(qt[1:], fq[1:])
    r_err = float(2.0 * np.arctan2(np.linalg.norm(vec), abs(w)))
    out.update({f"{name}/vertices": v, f"{name}/faces": f, f"{name}/points": points, f"{name}/init_position": init_pose[0],
                f"{name}/init_quaternion": init_pose[1], f"{name}/true_position": truth[0], f"{name}/true_quaternion": truth[1],
                f"{name}/final_error": np.array([t_err, r_err]),
                f"{name}/params": np.array([cfg.distance_threshold, cfg.max_distance, float(cfg.use_huber), cfg.huber_delta, cfg.lambda_initial,
                                            cfg.lambda_factor, cfg.lambda_min, cfg.lambda_max, cfg.rho_min], np.float64)})
    print(name, "final translation error", t_err, "rotation error", r_err)


def sequences(out):
    rng = np.random.default_rng(77)
    v, f = l_solid()
    truth = GENERAL
    off = Pose.from_euler_xyz(torch.tensor([0.05, -0.04, 0.035]), torch.tensor([0.012, -0.011, 0.0115]))  # ~5 deg, 2 cm
    init = off.multiply(Pose(position=torch.as_tensor(truth[0])[None], quaternion=torch.as_tensor(truth[1])[None]))
    init = (init.position[0].numpy().astype(np.float32), init.quaternion[0].numpy().astype(np.float32))
    n = 400
    s, nrm = surface_samples(v, f, n, rng)
    clean = to_world(s.astype(np.float32), truth)
    noisy_m = s + rng.normal(0, 0.001, s.shape)
    k = rng.choice(n, n // 20, replace=False)
    noisy_m[k] = s[k] + nrm[k] * rng.uniform(0.05, 0.15, (len(k), 1))
    noisy = to_world(noisy_m.astype(np.float32), truth)
    cfg = SDFDetectorCfg(use_cuda_graph=False, n_points=n)
    names = []
    for name, pts in (("seq_clean", clean), ("seq_noisy", noisy)):
        run_sequence(out, name, v, f, pts, init, truth, cfg, 25)
        names.append(name)
    # short sequences at the edges of the trust-region update: a rank-deficient system, 10 and 11 valid points
    e = {c[0]: c for c in EVAL_CASES}
    for name, case in (("seq_singular", "plane_singular"), ("seq_valid10", "lsolid_valid10"), ("seq_valid11", "lsolid_valid11")):
        _, _, pose, _, thr, huber, _ = e[case]
        c = SDFDetectorCfg(use_cuda_graph=False, distance_threshold=thr, use_huber=huber is not None, huber_delta=huber or 0.1)
        start = (pose[0] + np.float32(0.003), pose[1])
        run_sequence(out, name, out[f"{case}/vertices"], out[f"{case}/faces"], out[f"{case}/points"], start, pose, c, 4)
        names.append(name)
    out["sequence_names"] = np.array(names)


def main():
    out = {}
    eval_cases(out)
    sequences(out)
    defaults = {fl.name: getattr(SDFDetectorCfg(), fl.name) for fl in dataclasses.fields(SDFDetectorCfg) if fl.name != "device_cfg"}
    out["cfg_default_names"] = np.array(list(defaults))
    out["cfg_default_values"] = np.array([float(x) for x in defaults.values()], np.float64)
    path = os.path.join(HERE, "pose_detector_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
