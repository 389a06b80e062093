"""Times of the ICP pose detector at its default configuration (csrc/pose_icp.hip; 64 hypotheses, 500 / 2000 coarse, 2000 / 10000
fine, 50 iterations each) -> <out>/pose_icp_timing.jsonl, and a paragraph appended to docs/NOTEBOOK.md.

    python tools/pose_icp_timing.py [--out profiles] [--torch-reps 2]

Per stage: ms per replay of the stage's captured graph (device events around repeated replays after a warm-up, median of the
rounds), us per iteration inside it, and the same loop restated in plain torch on the same GPU (the hypotheses one after the
other, cdist / min / gather / J^T J / cholesky per iteration, as the reference writes it).  The synthetic object is a scalene
tetrahedron seen without noise; both forms get the same samples, observations and rotations."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from curobo_amd.backends import perception as P  # noqa: E402
from curobo_amd.perception.pose_estimation import DetectorCfg, PoseDetector, RobotMesh  # noqa: E402

DEV = "cuda:0"
V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * np.array([0.3, 0.2, 0.12], np.float32)
F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def timed(fn, reps, rounds=5, warmup=3):
    for _ in range(warmup):
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
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def torch_stage(T0, mesh_points, mesh_normals, observed, n_iterations, threshold, delta, fine):
    """the reference's loop in plain torch, every hypothesis in turn -> (transforms, errors)"""
    eye = torch.eye(6, device=DEV)
    out_T, out_e = [], []
    for T in T0:
        T = T.clone()
        for _ in range(n_iterations):
            s = mesh_points @ T[:3, :3].T + T[:3, 3]
            n = mesh_normals @ T[:3, :3].T
            d, idx = torch.cdist(s.unsqueeze(0), observed.unsqueeze(0)).squeeze(0).min(dim=1)
            ok = d <= threshold
            if ok.sum() < 10:
                break
            s, n, o = s[ok], n[ok], observed[idx[ok]]
            b = ((o - s) * n).sum(1)
            w = torch.where(b.abs() < delta, torch.ones_like(b), delta / (b.abs() + 1e-10))
            J = torch.cat([torch.cross(s, n, dim=1), n], 1) * w.sqrt().unsqueeze(1)
            L, info = torch.linalg.cholesky_ex(J.T @ J + 1e-6 * eye)
            x = torch.cholesky_solve((J.T @ (b * w.sqrt())).unsqueeze(1), L).squeeze(1)
            theta = x[:3].norm()
            q = torch.cat([torch.cos(0.5 * theta).unsqueeze(0), x[:3] * (torch.sin(0.5 * theta) / theta.clamp(min=1e-10))])
            qw, qx, qy, qz = q
            U = torch.eye(4, device=DEV)
            U[:3, :3] = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                                     2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                                     2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]).reshape(3, 3)
            U[:3, 3] = x[3:]
            if fine and x[3:].norm().item() < 1e-4:
                break
            T = U @ T
        s = mesh_points @ T[:3, :3].T + T[:3, 3]
        out_e.append(torch.cdist(s.unsqueeze(0), observed.unsqueeze(0)).squeeze(0).min(dim=1)[0].mean().item())
        out_T.append(T)
    return out_T, out_e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--torch-reps", type=int, default=2)
    args = ap.parse_args()
    torch.manual_seed(0)
    cfg = DetectorCfg()
    mesh = RobotMesh(V, F, device=DEV)
    det = PoseDetector(mesh, cfg)
    # the object seen at a pose, 12 000 points
    rng = np.random.default_rng(0)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rt = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    seen, _ = mesh.sample_surface_points(12000)
    observed = seen @ torch.as_tensor(Rt, dtype=torch.float32, device=DEV).T + torch.tensor([0.31, -0.12, 0.45], device=DEV)
    result = det.detect_from_points(observed)  # records both graphs
    torch.cuda.synchronize()
    rows = []
    for mode, name in ((P.POSE_ICP_COARSE, "coarse"), (P.POSE_ICP_FINE, "fine")):
        st = next(s for key, s in det._stages.items() if key[0] == mode)
        start = st.state.clone()
        start[:, P.pose_icp_state_slice("error").start:] = 0.0
        n_it = cfg.n_iterations_coarse if name == "coarse" else cfg.n_iterations_fine
        thr = cfg.distance_threshold_coarse if name == "coarse" else cfg.distance_threshold_fine

        def replay():
            st.state.copy_(start)  # (every replay starts from the stage's start: running hypotheses, not stopped ones)
            st.graph.replay()
        # the start transforms: the coarse stage's own random starts are gone from the state, so draw them again
        if name == "coarse":
            T0 = torch.eye(4, device=DEV).repeat(st.h, 1, 1)
            T0[:, :3, :3] = det._sample_rotations(st.h)
            T0[:, :3, 3] = st.observed.mean(dim=0)
        else:
            T0 = torch.eye(4, device=DEV).repeat(1, 1, 1)
            T0[0, :3, :] = det._stages[next(k for k in det._stages if k[0] == P.POSE_ICP_COARSE)].best_transform.reshape(3, 4)
        start[:, :12] = T0[:, :3, :].reshape(st.h, 12)
        med, lo, hi = timed(replay, reps=10)
        t_med, t_lo, t_hi = timed(lambda: torch_stage(T0, st.mesh_points, st.mesh_normals, st.observed, n_it, thr, cfg.huber_delta, name == "fine"),
                                  reps=1, rounds=args.torch_reps, warmup=1)
        replay()
        torch.cuda.synchronize()
        iterations = st.field("iterations")[:, 0].cpu().numpy()
        rows.append(dict(stage=name, hypotheses=st.h, mesh_points=st.m, observed_points=st.o, iterations=n_it, graph_ms=med, graph_ms_min=lo,
                         graph_ms_max=hi, graph_us_per_iteration=med * 1e3 / n_it, iterations_run_mean=float(iterations.mean()),
                         torch_loop_ms=t_med, torch_loop_ms_min=t_lo, torch_loop_ms_max=t_hi, speedup=t_med / med))
        print(rows[-1])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "pose_icp_timing.jsonl"), "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    c, f = rows
    verdict = lambda r: "faster" if r["speedup"] > 1 else "NOT faster"  # noqa: E731
    text = (f"\n**ICP pose detector, default configuration (`tools/pose_icp_timing.py`, device events, median of 5 x 10 graph replays; the torch loop "
            f"median of {args.torch_reps}).**  Coarse stage ({c['hypotheses']} hypotheses, {c['mesh_points']} / {c['observed_points']} points, "
            f"{c['iterations']} iterations + final error + selection, one graph): {c['graph_ms']:.3f} ms per replay ({c['graph_ms_min']:.3f}-"
            f"{c['graph_ms_max']:.3f}), {c['graph_us_per_iteration']:.1f} us per iteration of all hypotheses; the same loop in plain torch on the same "
            f"GPU, hypothesis after hypothesis: {c['torch_loop_ms']:.1f} ms -- the graph is {verdict(c)} ({c['speedup']:.1f} x).  Fine stage (1 hypothesis, "
            f"{f['mesh_points']} / {f['observed_points']} points, {f['iterations']} iterations recorded, {f['iterations_run_mean']:.0f} run before the "
            f"translation stop): {f['graph_ms']:.3f} ms per replay ({f['graph_ms_min']:.3f}-{f['graph_ms_max']:.3f}); torch loop {f['torch_loop_ms']:.1f} ms "
            f"-- the graph is {verdict(f)} ({f['speedup']:.1f} x; the torch loop leaves at its break, the graph replays every recorded launch, stopped "
            f"ones returning at once).  Whole `detect_from_points` at this configuration: {result.compute_time * 1e3:.1f} ms the first time "
            f"(records both graphs).\n")
    with open(os.path.join(args.out, "pose_icp_timing.md"), "w") as fh:
        fh.write(text)
    with open(os.path.join(ROOT, "docs", "NOTEBOOK.md"), "a") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
