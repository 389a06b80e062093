"""Golden vectors for the point-to-plane ICP detector (csrc/pose_icp.hip, curobo_amd/perception/pose_estimation/pose_detector.py),
produced by the REFERENCE's own code on the CPU:

    PYTHONPATH=/root/reference python tests/golden/make_pose_icp_golden.py

``PoseDetector._icp_coarse`` and ``PoseDetector._icp_fine`` (pose_detector.py) run unmodified, with ``find_nearest_neighbors`` and
``compute_pose_point_to_plane_cholesky`` (util.py) wrapped only to RECORD their arguments and results.  The random parts are
injected -- the mesh samples, the resampled observations and the rotations are drawn HERE, rounded to fp32 and recorded -- so a
run in fp32 and a run in float64 see identical inputs.  The transform of every iteration is not handed to the two functions;
it is rebuilt here as the reference builds it (``T_update @ T_current``, same dtype, same operations) and PROVED to be the
reference's by the next call's arguments: the transformed mesh must match bit for bit.  Likewise the 28 sums and the solve are
recomputed by the reference's formulas and the translation must match what its solver returned.

float64: the reference's ``Pose.get_matrix`` accepts fp32 only, so in the float64 run ``Pose`` is replaced, inside the
detector's module, by a two-line stand-in over the reference's own ``torch_quaternion_to_matrix`` (geom/transform.py).

Configuration: the reference test's (200 / 500 / 8 / 10 / 0.1 coarse, 500 / 1000 / 20 / 0.02 fine, Huber 0.02).  Mesh: the
scalene tetrahedron of tests/test_pose_detector_host.py scaled to 0.3 x 0.2 x 0.12 m (no symmetry); observations noise-free
from its surface at a known pose.  The seed is the first that passes the assertions below, which are made BEFORE writing:
both runs end within 1 mm and 0.5 deg of the truth, the winning coarse error is below 0.75 x the runner-up's, and at most 2 %
of the samples of any recorded iteration are in the oracle's excluded set.

Output: tests/golden/pose_icp_golden.npz -- arrays, names and cfg values only."""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reference_robot_loader as _R  # noqa: E402,F401  (the Warp stand-in, the stubs, DeviceCfg held to the CPU)
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import pose_icp_ref as ORACLE  # noqa: E402  (tests/pose_icp_ref.py: its excluded set and pose error)

import curobo._src.perception.pose_estimation.pose_detector as PD  # noqa: E402
from curobo._src.geom.transform import torch_quaternion_to_matrix  # noqa: E402
from curobo._src.types.device_cfg import DeviceCfg  # noqa: E402

V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) * [0.3, 0.2, 0.12]
F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
CFG = dict(n_mesh_points_coarse=200, n_observed_points_coarse=500, n_rotation_samples=8, n_iterations_coarse=10, distance_threshold_coarse=0.1,
           n_mesh_points_fine=500, n_observed_points_fine=1000, n_iterations_fine=20, distance_threshold_fine=0.02, use_huber_loss=True,
           huber_delta=0.02)
N_OBSERVED = 800  # fewer than the fine stage asks for: resample_points repeats points, as it does on a small segment


class _Pose64:
    """``Pose(position, quaternion).get_matrix()`` for the float64 run"""

    def __init__(self, position, quaternion):
        self.position, self.quaternion = position, quaternion

    def get_matrix(self):
        m = torch.eye(4, dtype=self.position.dtype).repeat(len(self.position), 1, 1)
        m[:, :3, :3] = torch_quaternion_to_matrix(self.quaternion)
        m[:, :3, 3] = self.position
        return m


def surface(n, rng):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    k = rng.choice(len(F), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    p = (1 - r1)[:, None] * a[k] + (r1 * (1 - r2))[:, None] * b[k] + (r1 * r2)[:, None] * c[k]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p.astype(np.float32), nrm[k].astype(np.float32)


def shoemake(n, rng):
    u = rng.uniform(0, 1, (n, 3))
    w, x = np.sqrt(1 - u[:, 0]) * np.sin(2 * np.pi * u[:, 1]), np.sqrt(1 - u[:, 0]) * np.cos(2 * np.pi * u[:, 1])
    y, z = np.sqrt(u[:, 0]) * np.sin(2 * np.pi * u[:, 2]), np.sqrt(u[:, 0]) * np.cos(2 * np.pi * u[:, 2])
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    return R.astype(np.float32)


def draw(seed):
    rng = np.random.default_rng(seed)
    T_true = np.eye(4)
    T_true[:3, :3] = shoemake(1, rng)[0].astype(np.float64)
    T_true[:3, 3] = [0.31, -0.12, 0.45]
    s, _ = surface(N_OBSERVED, rng)
    raw = (s.astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3]).astype(np.float32)
    inj = {"T_true": T_true, "observed_raw": raw, "rotations": shoemake(CFG["n_rotation_samples"], rng)}
    for stage in ("coarse", "fine"):
        m, o = CFG[f"n_mesh_points_{stage}"], CFG[f"n_observed_points_{stage}"]
        inj[f"{stage}_mesh_points"], inj[f"{stage}_mesh_normals"] = surface(m, rng)
        reps = np.tile(raw, (o // len(raw) + 1, 1)) if len(raw) < o else raw
        inj[f"{stage}_observed"] = reps[rng.permutation(len(reps))[:o]]
    return inj


class _Geometry:
    def __init__(self, inj, dtype):
        self.inj, self.dtype = inj, dtype

    def get_dof(self):
        return 0

    def sample_surface_points(self, n):
        stage = "coarse" if n == CFG["n_mesh_points_coarse"] else "fine"
        return torch.as_tensor(self.inj[f"{stage}_mesh_points"]).to(self.dtype), torch.as_tensor(self.inj[f"{stage}_mesh_normals"]).to(self.dtype)


def reference_sums(src, tgt, nrm, delta, dtype):
    """compute_pose_point_to_plane_cholesky (util.py:279-321), line for line, keeping what it throws away"""
    diff = tgt - src
    distances = (diff * nrm).sum(dim=1)
    abs_dist = distances.abs()
    weights = torch.where(abs_dist < delta, torch.ones_like(abs_dist), delta / (abs_dist + 1e-10))
    cross = torch.cross(src, nrm, dim=1)
    sqrt_w = weights.sqrt().unsqueeze(1)
    J = torch.cat([cross * sqrt_w, nrm * sqrt_w], dim=1)
    b = distances * sqrt_w.squeeze(1)
    JtJ, Jtb = J.T @ J, J.T @ b
    L, info = torch.linalg.cholesky_ex(JtJ + 1e-6 * torch.eye(6, dtype=dtype))
    assert info == 0
    x = torch.cholesky_solve(Jtb.unsqueeze(1), L).squeeze(1)
    return JtJ, Jtb, x


def run(inj, dtype):
    """the reference's two stages on the injected inputs -> the record of every iteration"""
    log = []
    real_nn, real_solve, real_resample, real_pose = PD.find_nearest_neighbors, PD.compute_pose_point_to_plane_cholesky, PD.resample_points, PD.Pose

    def nn(source, target, distance_threshold=float("inf")):
        idx = real_nn(source, target, distance_threshold=distance_threshold)
        # the distances as the reference's final error takes them (pose_detector.py:269): the norm of the differences to the
        # nearest points -- cdist's own fp32 values come from an expanded square and are far coarser
        nearest = torch.cdist(source.unsqueeze(0), target.unsqueeze(0)).squeeze(0).min(dim=1)[1]
        dist = torch.norm(source - target[nearest], dim=1)
        log.append(dict(kind="nn", source=source.clone(), index=idx.clone(), threshold=distance_threshold, sum_dist=dist.sum().item()))
        return idx

    def solve(src, tgt, nrm, use_huber=False, huber_delta=0.02):
        pos, quat = real_solve(src, tgt, nrm, use_huber=use_huber, huber_delta=huber_delta)
        log.append(dict(kind="solve", src=src.clone(), tgt=tgt.clone(), nrm=nrm.clone(), position=pos.clone(), quaternion=quat.clone()))
        return pos, quat

    def resample(points, n, device=None):
        stage = "coarse" if n == CFG["n_observed_points_coarse"] else "fine"
        return torch.as_tensor(inj[f"{stage}_observed"]).to(dtype)

    PD.find_nearest_neighbors, PD.compute_pose_point_to_plane_cholesky, PD.resample_points = nn, solve, resample
    if dtype == torch.float64:
        PD.Pose = _Pose64
    try:
        det = PD.PoseDetector(_Geometry(inj, dtype), PD.DetectorCfg(**CFG, device_cfg=DeviceCfg(dtype=dtype)))
        det._sample_rotations = lambda n: torch.as_tensor(inj["rotations"]).to(dtype)
        raw = torch.as_tensor(inj["observed_raw"]).to(dtype)
        T_coarse, err_coarse, best, _ = det._icp_coarse(raw, None)
        n_coarse = len(log)
        T_fine, err_fine, n_iter, _ = det._icp_fine(T_coarse, raw, None)
        pose_cls = PD.Pose
    finally:
        PD.find_nearest_neighbors, PD.compute_pose_point_to_plane_cholesky, PD.resample_points, PD.Pose = real_nn, real_solve, real_resample, real_pose

    def replay(entries, stage, starts, fine):
        """walk the log of one stage; rebuild T; prove it by the recorded arguments"""
        mesh = torch.as_tensor(inj[f"{stage}_mesh_points"]).to(dtype)
        n_it, m = CFG[f"n_iterations_{stage}"], len(mesh)
        h = len(starts)
        rec = dict(T_before=np.zeros((h, n_it, 12)), T_after=np.zeros((h, n_it, 12)), rows=np.zeros((h, n_it, 28)), x=np.zeros((h, n_it, 6)),
                   count=np.zeros((h, n_it), np.int32), index=np.full((h, n_it, m), -1, np.int32), ran=np.zeros((h, n_it), bool),
                   solved=np.zeros((h, n_it), bool), error=np.zeros(h), T_final=np.zeros((h, 12)), iterations=np.zeros(h, np.int32))
        k = 0
        for i, T in enumerate(starts):
            T = T.clone()
            for it in range(n_it):
                e = entries[k]
                if e["kind"] != "nn" or e["threshold"] == float("inf"):
                    break  # the loop ended early (a break in the iteration before)
                k += 1
                assert torch.equal(e["source"], (T[:3, :3] @ mesh.T).T + T[:3, 3]), (stage, i, it, "the rebuilt transform is not the reference's")
                rec["ran"][i, it], rec["T_before"][i, it], rec["index"][i, it] = True, T[:3].reshape(-1).numpy(), e["index"].numpy()
                rec["count"][i, it], rec["iterations"][i] = int((e["index"] >= 0).sum()), it + 1
                rec["rows"][i, it, 27] = e["sum_dist"]
                rec["T_after"][i, it] = T[:3].reshape(-1).numpy()
                if rec["count"][i, it] < 10:
                    break
                s = entries[k]
                k += 1
                assert s["kind"] == "solve"
                JtJ, Jtb, x = reference_sums(s["src"], s["tgt"], s["nrm"], CFG["huber_delta"], dtype)
                assert torch.equal(x[3:], s["position"]), (stage, i, it, x[3:], s["position"])
                rec["rows"][i, it, :21], rec["rows"][i, it, 21:27] = JtJ[np.triu_indices(6)].numpy(), Jtb.numpy()
                rec["x"][i, it], rec["solved"][i, it] = x.numpy(), True
                T_update = pose_cls(position=s["position"].unsqueeze(0), quaternion=s["quaternion"].unsqueeze(0)).get_matrix().squeeze(0)
                if fine and torch.norm(T_update[:3, 3]).item() < 1e-4:
                    break
                T = T_update @ T
                rec["T_after"][i, it] = T[:3].reshape(-1).numpy()
            e = entries[k]
            k += 1
            assert e["kind"] == "nn" and e["threshold"] == float("inf")
            assert torch.equal(e["source"], (T[:3, :3] @ mesh.T).T + T[:3, 3]), (stage, i, "final transform")
            rec["T_final"][i] = T[:3].reshape(-1).numpy()
            rec["error"][i] = e["sum_dist"] / m  # (errors.mean())
        assert k == len(entries), (stage, k, len(entries))
        return rec

    obs_mean = torch.as_tensor(inj["coarse_observed"]).to(dtype).mean(dim=0, keepdim=True)
    starts = []
    for R in torch.as_tensor(inj["rotations"]).to(dtype):
        T = torch.eye(4, dtype=dtype)
        T[:3, :3] = R
        T[:3, 3] = obs_mean.squeeze()
        starts.append(T)
    coarse = replay(log[:n_coarse], "coarse", starts, False)
    fine = replay(log[n_coarse:], "fine", [T_coarse], True)
    assert np.array_equal(coarse["T_final"][best], T_coarse[:3].reshape(-1).numpy()) and np.array_equal(fine["T_final"][0], T_fine[:3].reshape(-1).numpy())
    assert fine["iterations"][0] == n_iter and abs(coarse["error"][best] - err_coarse) < 1e-6 and int(np.argmin(coarse["error"])) == best
    return dict(coarse=coarse, fine=fine, best=best, err_coarse=err_coarse, err_fine=err_fine, T_final=T_fine[:3].numpy().astype(np.float64),
                n_iter=n_iter)


def excluded_share(inj, rec, stage):
    """the largest share of excluded samples over the recorded iterations, and the reference's index mismatches outside it"""
    worst = 0.0
    for i, it in zip(*np.nonzero(rec["ran"])):
        c = ORACLE.correspond(inj[f"{stage}_mesh_points"], inj[f"{stage}_mesh_normals"], inj[f"{stage}_observed"], rec["T_before"][i, it],
                              CFG[f"distance_threshold_{stage}"], True, CFG["huber_delta"])
        worst = max(worst, float(c["excluded"].mean()))
    return worst


def main():
    for seed in range(100):
        inj = draw(seed)
        runs = {name: run(inj, dt) for name, dt in (("fp32", torch.float32), ("fp64", torch.float64))}
        errs = {name: ORACLE.pose_error(r["T_final"], inj["T_true"][:3]) for name, r in runs.items()}
        ratio = {name: np.sort(r["coarse"]["error"])[0] / np.sort(r["coarse"]["error"])[1] for name, r in runs.items()}
        print("seed", seed, {k: (f"{v[0] * 1e3:.3f} mm", f"{np.degrees(v[1]):.3f} deg") for k, v in errs.items()}, "coarse winner / runner-up", ratio,
              "best", {k: r["best"] for k, r in runs.items()})
        if not all(e[0] < 1e-3 and e[1] < np.radians(0.5) for e in errs.values()) or not all(v < 0.75 for v in ratio.values()):
            continue
        if runs["fp32"]["best"] != runs["fp64"]["best"]:
            continue
        share = max(excluded_share(inj, runs[n][s], s) for n in runs for s in ("coarse", "fine"))
        print("  excluded share", share)
        if share > 0.02:
            continue
        break
    else:
        raise SystemExit("no seed passes the assertions")
    assert all(e[0] < 1e-3 and e[1] < np.radians(0.5) for e in errs.values()) and all(v < 0.75 for v in ratio.values()) and share <= 0.02
    out = {"seed": np.array(seed), "vertices": V.astype(np.float32), "faces": F, "T_true": inj["T_true"][:3], "observed_raw": inj["observed_raw"],
           "rotations": inj["rotations"], "excluded_share": np.array(share)}
    for stage in ("coarse", "fine"):
        for k in ("mesh_points", "mesh_normals", "observed"):
            out[f"{stage}_{k}"] = inj[f"{stage}_{k}"]
    for name, r in runs.items():
        for stage in ("coarse", "fine"):
            for k, v in r[stage].items():
                out[f"{name}/{stage}/{k}"] = v.astype(np.float32) if name == "fp32" and v.dtype == np.float64 else v
        out[f"{name}/best_hypothesis"], out[f"{name}/n_iterations"] = np.array(r["best"]), np.array(r["n_iter"])
        out[f"{name}/final_error"], out[f"{name}/T_final"] = np.array(errs[name]), r["T_final"]
        out[f"{name}/alignment_error"] = np.array([r["err_coarse"], r["err_fine"]])
    out["cfg_names"] = np.array(list(CFG))
    out["cfg_values"] = np.array([float(v) for v in CFG.values()], np.float64)
    defaults = {fl.name: getattr(PD.DetectorCfg(), fl.name) for fl in dataclasses.fields(PD.DetectorCfg) if fl.name != "device_cfg"}
    out["cfg_default_names"] = np.array(list(defaults))
    out["cfg_default_values"] = np.array([float(x) for x in defaults.values()], np.float64)
    path = os.path.join(HERE, "pose_icp_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
