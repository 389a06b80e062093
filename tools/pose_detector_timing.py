"""Times of the pose-refinement launches at N = 5000 (csrc/pose_detect.hip) -> profiles/pose_detector_timing.jsonl.

    python tools/pose_detector_timing.py

On an L-shaped solid of 28 triangles and on an icosphere of 20 480 triangles: us per evaluate launch, per LM iteration
(evaluate + step) eager and inside the captured block, per whole 25-iteration block, and the same J^T J built from the pieces
the library had before (``mesh_query`` + a torch reduction).  Device events around many launches after a warm-up, one process."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from curobo_amd.backends import perception as P  # noqa: E402
from curobo_amd.backends.mesh import mesh_query  # noqa: E402
from curobo_amd.perception import RobotMesh, SDFDetectorCfg, SDFPoseDetector  # noqa: E402
from curobo_amd.perception.pose_estimation.sdf_pose_detector import _Run  # noqa: E402

DEV = "cuda:0"


def icosphere(levels, radius=0.1):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []
        for a, b, c in f:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in mid:
                    p = v[i] + v[j]
                    v.append(p / np.linalg.norm(p))
                    mid[key] = len(v) - 1
                m.append(mid[key])
            nf += [[a, m[0], m[2]], [b, m[1], m[0]], [c, m[2], m[1]], m]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def timed(fn, reps=200, rounds=5):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out))


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_detector_golden.npz"))
    rng = np.random.default_rng(0)
    rows = []
    for name, (v, f) in (("lsolid_28", (g["seq_clean/vertices"], g["seq_clean/faces"])), ("icosphere_20480", icosphere(5))):
        n = 5000
        k = rng.integers(0, len(f), n)
        w = rng.dirichlet([1, 1, 1], n)
        pts = (v[f[k]].astype(np.float64) * w[:, :, None]).sum(1) + rng.normal(0, 0.002, (n, 3))
        det = SDFPoseDetector(RobotMesh(v, f, device=DEV), SDFDetectorCfg())
        run = _Run(n, torch.device(DEV))
        run.points.copy_(torch.as_tensor(pts, dtype=torch.float32))
        run.field("cand_position").copy_(torch.tensor([0.004, -0.003, 0.002]))
        run.field("cand_quaternion").copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
        det._evaluate(run)
        det._step(run, P.POSE_LM_INIT)
        saved = run.state.clone()
        ev = timed(lambda: det._evaluate(run))

        def iteration():
            det._evaluate(run)
            det._step(run, P.POSE_LM_UPDATE)
        eager = timed(iteration)
        run.state.copy_(saved)
        det._run_block(run)  # records the graph
        block = timed(lambda: run.graph.replay(), reps=20)
        mesh = det.robot_mesh.device_mesh
        p = run.points

        def composed():  # the parent's pieces: mesh_query (signed, mesh frame) + the Jacobian and its products in torch
            sdf, grad = mesh_query(mesh, p, 0.2)
            d = sdf.abs()
            ok = (d <= 0.2) & (d > 1e-8)
            gw = -grad * torch.sign(sdf).unsqueeze(1)
            J = torch.cat([gw, torch.cross(p, gw, dim=1)], 1) * ok.unsqueeze(1)
            return J.T @ J, J.T @ (d * ok), (d * ok).square().sum(), ok.sum()
        comp = timed(composed, reps=50)
        rows.append(dict(mesh=name, triangles=int(len(f)), n_points=n, evaluate_us=ev, iteration_eager_us=eager, block_of_25_captured_us=block,
                         iteration_captured_us=block / det.config.inner_iterations, composed_mesh_query_plus_torch_us=comp,
                         eight_lane_walk_us=None))
        print(rows[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_detector_timing.jsonl"), "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
