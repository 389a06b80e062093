"""Randomised parity of the pose-refinement evaluation (csrc/pose_detect.hip) against the float64 oracle tests/pose_detector_ref.py:

    python tests/randomised/fuzz_pose_detector.py <cases> <seed>

Random triangle soups of 1-400 triangles, poses, 1-6000 points, thresholds and Huber settings; the rules of
tests/test_gpu_pose_detector.py: valid equal, distance and gradient inside the bounds of the oracle outside its excluded set
(at most 1 % of a case), the reduced sums inside (N + 8) 2^-24 sum |term| of the float64 sums of the kernel's own per-point
outputs, the count exact.  Exit status 0 when every case passes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import pose_detector_ref as R  # noqa: E402
import pose_rows  # noqa: E402


def hip_evaluate(points, position, quaternion, vertices, faces, max_distance, threshold, use_huber, delta, device="cuda:0"):
    """one launch with every per-point output; returns numpy arrays and the reduced row sums (float64 sums of the rows, count)"""
    from curobo_amd.backends import perception as P
    from curobo_amd.backends.mesh import build_mesh_bvh

    mesh = build_mesh_bvh(vertices, faces, device, cells=False)
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt).contiguous()  # noqa: E731
    pts = t(points)
    n = len(pts)
    ws = torch.full((P.pose_sdf_ws_bytes(n) // 4,), float("nan"), device=device)
    dist, grad, valid = torch.full((n,), -1.0, device=device), torch.full((n, 3), -1.0, device=device), torch.full((n,), -1, dtype=torch.int32, device=device)
    P.pose_sdf_evaluate(ws, pts, t(position), t(quaternion), mesh.struct, max_distance, threshold, use_huber, delta, dist, grad, valid)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), grad.cpu().numpy(), valid.cpu().numpy(), ws.cpu().numpy().reshape(-1, P.POSE_WS_ROW)


def reduce_rows(rows):
    """(JtJ [6, 6], Jtr, sum_sq, n) of the workspace rows, the rows added in fp32 in order as the step kernel adds them"""
    acc, n = pose_rows.reduce_rows(rows)
    return (*pose_rows.unpack_row(acc), float(acc[27]), n)


def check_case(name, points, position, quaternion, vertices, faces, max_distance, threshold, use_huber, delta, say=print):
    """the per-point and the reduction rules on one case; returns a list of failures"""
    dist, grad, valid, rows = hip_evaluate(points, position, quaternion, vertices, faces, max_distance, threshold, use_huber, delta)
    ev = R.evaluate(points, position, quaternion, vertices, faces, float(np.float32(max_distance)), float(np.float32(threshold)), use_huber,
                    float(np.float32(delta)))
    bad = []
    keep = ~ev["excluded"]
    if ev["excluded"].mean() > 0.01:
        bad.append(f"excluded share {ev['excluded'].mean():.4f}")
    if not np.array_equal(valid.astype(bool)[keep], ev["valid"][keep]):
        bad.append(f"valid differs at {np.flatnonzero((valid.astype(bool) != ev['valid']) & keep)[:5]}")
    if not set(np.unique(valid)) <= {0, 1}:
        bad.append("valid is not 0 / 1")
    inv = valid == 0
    if (dist[inv] != 0).any() or (grad[inv] != 0).any():
        bad.append("invalid points carry values")
    tol_d, tol_g = R.point_bounds(ev)
    m = keep & ev["valid"] & (valid == 1)
    ed, eg = np.abs(dist - ev["dist"]), np.abs(grad - ev["grad"]).max(1)
    rd, rg = (float((ed[m] / tol_d[m]).max()), float((eg[m] / tol_g[m]).max())) if m.any() else (0.0, 0.0)
    if rd > 1 or rg > 1:
        bad.append(f"distance {rd:.3f} / gradient {rg:.3f} of the bound")
    # the reduction, against the float64 sums of the kernel's OWN per-point outputs
    J, r, v = R.jacobian_from_outputs(points, dist, grad, valid, use_huber, delta)
    s = R.sums_of(J, r, v)
    JtJ, Jtr, ssq, cnt = reduce_rows(rows)
    # (the kernel forms each Jacobian entry in fp32 before it multiplies: 4 roundings per entry on top of the summation)
    bound = lambda term: pose_rows.row_bound(len(r), s[term], 8) + 1e-45  # noqa: E731
    worst = max(float((np.abs(JtJ - s["JtJ"]) / bound("abs_JtJ")).max()), float((np.abs(Jtr - s["Jtr"]) / bound("abs_Jtr")).max()),
                abs(ssq - s["sum_sq"]) / bound("abs_sum_sq"))
    if worst > 1:
        bad.append(f"reduced sums at {worst:.3f} of the bound")
    if cnt != s["n"]:
        bad.append(f"count {cnt} != {s['n']}")
    if s["n"] == 0 and (JtJ.any() or Jtr.any() or ssq != 0.0):
        bad.append("zero valid points but non-zero sums")
    say(f"{name}: N {len(points)} triangles {len(faces)} valid {cnt} excluded {int(ev['excluded'].sum())} distance {rd:.3f} gradient {rg:.3f} "
        f"sums {worst:.3f} of their bounds{'  FAIL ' + '; '.join(bad) if bad else ''}")
    return bad


def random_case(rng):
    n_tri = int(rng.choice([1, 2, 7, 8, 9, 16, 17, int(rng.integers(1, 401))]))
    centres = rng.uniform(-0.3, 0.3, (n_tri, 1, 3))
    vertices = (centres + rng.normal(0, 0.06, (n_tri, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_tri, dtype=np.int32).reshape(-1, 3)
    n = int(rng.choice([1, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 6001))]))
    thr = float(rng.choice([0.02, 0.05, 0.2]))
    k = rng.integers(0, n_tri, n)
    w = rng.dirichlet([1, 1, 1], n)
    base = (vertices[faces[k]].astype(np.float64) * w[:, :, None]).sum(1)
    d = rng.normal(size=(n, 3))
    pm = base + d / np.linalg.norm(d, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(1e-3), np.log(2.5 * thr), n))[:, None]
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    t = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
    pts = (R.quat_rotate(q.astype(np.float64), pm) + t).astype(np.float32)
    huber = bool(rng.integers(0, 2))
    return dict(points=pts, position=t, quaternion=q, vertices=vertices, faces=faces, max_distance=thr, threshold=thr, use_huber=huber,
                delta=float(rng.choice([0.3, 0.6])) * thr)


def main(cases, seed):
    rng = np.random.default_rng(seed)
    failed = 0
    for c in range(cases):
        failed += bool(check_case(f"case {c}", **random_case(rng)))
    print(f"fuzz_pose_detector: {cases - failed} of {cases} cases passed (seed {seed})")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]), int(sys.argv[2])))
