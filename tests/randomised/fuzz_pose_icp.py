"""Randomised parity of the ICP correspondence launch (csrc/pose_icp.hip) against the float64 oracle tests/pose_icp_ref.py:

    python tests/randomised/fuzz_pose_icp.py <cases> <seed>

Random meshes, poses, H, M, O, thresholds and Huber settings, and degenerate inputs: coincident observed points, every
observation beyond the threshold, fewer than ten observations.  The rules of tests/test_gpu_pose_icp.py: per sample the nearest
index exact and the distance inside the oracle's bound outside its excluded set (at most 2 % of a hypothesis), the rows inside
(N + 24) 2^-24 sum |term| of the float64 sums over the kernel's own correspondences, the count exact; then one step per
hypothesis inside the K bound (stopped for fewer than ten valid samples; finite and nothing more where the random system is
singular in fp32, cond 2^-24 >= 0.1).  Exit status 0 when every case passes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import pose_icp_ref as R  # noqa: E402
from pose_rows import reduce_rows  # noqa: E402

DEV = "cuda:0"
#: cond(J^T J + 1e-6 I) 2^-24 from which a random system counts as singular in fp32: the K bound is a first-order one
SINGULAR = 0.1


def to_dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()


def make_state(T, stopped=None):
    """[H, POSE_ICP_STATE_WORDS] on the device from transforms [H, 12]"""
    from curobo_amd.backends import perception as P

    T = np.asarray(T, np.float32).reshape(-1, 12)
    st = np.zeros((len(T), P.POSE_ICP_STATE_WORDS), np.float32)
    st[:, P.pose_icp_state_slice("T")] = T
    if stopped is not None:
        st[:, P.pose_icp_state_slice("stopped")] = np.asarray(stopped, np.int32).reshape(-1, 1).view(np.float32)
    return to_dev(st)


def state_field(state, name):
    from curobo_amd.backends import perception as P

    return P.pose_state_field(state, P.PoseICPState, name).cpu().numpy()


def hip_correspond(mesh_points, mesh_normals, observed, T, threshold, use_huber, delta, stopped=None, honour_stopped=True, ws_fill=float("nan")):
    """one launch with both per-sample outputs -> (index [H, M], distance [H, M], rows [H, rows, 32], the state tensor, the workspace)"""
    from curobo_amd.backends import perception as P

    state = make_state(T, stopped)
    h, m = state.shape[0], len(mesh_points)
    ws = torch.full((P.pose_icp_ws_bytes(h, m) // 4,), ws_fill, device=DEV)
    idx = torch.full((h, m), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((h, m), -1.0, device=DEV)
    P.pose_icp_correspond(ws, to_dev(mesh_points), to_dev(mesh_normals), to_dev(observed), state, threshold, use_huber, delta,
                          honour_stopped=honour_stopped, out_index=idx, out_distance=dist)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), ws.cpu().numpy().reshape(h, -1, P.POSE_WS_ROW), state, ws


def check_case(name, mesh_points, mesh_normals, observed, T, threshold, use_huber, delta, say=print, step=True):
    """the per-sample, the reduction and the step rules on one case (every hypothesis); returns a list of failures"""
    from curobo_amd.backends import perception as P

    T = np.asarray(T, np.float32).reshape(-1, 12)
    idx, dist, rows, state, ws = hip_correspond(mesh_points, mesh_normals, observed, T, threshold, use_huber, delta)
    m, thr, dl = len(mesh_points), float(np.float32(threshold)), float(np.float32(delta))
    bad, worst_d, worst_r, worst_x, n_excluded = [], 0.0, 0.0, 0.0, 0
    if step:
        P.pose_icp_step(state, ws, m, P.POSE_ICP_COARSE)
        torch.cuda.synchronize()
        x_dev, T_dev, stopped, failed = (state_field(state, k) for k in ("x", "T", "stopped", "solver_failed"))
    for h in range(len(T)):
        c = R.correspond(mesh_points, mesh_normals, observed, T[h], thr, use_huber, dl)
        keep = ~c["excluded"]
        n_excluded += int(c["excluded"].sum())
        if c["excluded"].mean() > 0.02 and m >= 50:
            bad.append(f"h {h}: excluded share {c['excluded'].mean():.4f}")
        if not np.array_equal(idx[h][keep], c["index"][keep]):
            bad.append(f"h {h}: index differs at {np.flatnonzero((idx[h] != c['index']) & keep)[:5]}")
        tol = R.distance_bound(c["scale"], c["dist"])
        rd = float((np.abs(dist[h] - c["dist"]) / tol)[keep].max()) if keep.any() else 0.0
        worst_d = max(worst_d, rd)
        if rd > 1:
            bad.append(f"h {h}: distance at {rd:.3f} of the bound")
        if rows[h].shape[0] != -(-m // 64) or rows[h][:, 29:].any():
            bad.append(f"h {h}: row layout")
        # the reduction, against the float64 sums over the kernel's OWN correspondences
        own = R.correspond(mesh_points, mesh_normals, observed, T[h], thr, use_huber, dl, index=idx[h])
        acc, cnt = reduce_rows(rows[h])
        rr = float((np.abs(acc.astype(np.float64) - own["row"]) / (R.row_bound(m, own["row_abs"], R.ROW_ROUNDINGS_KERNEL) + 1e-45)).max())
        worst_r = max(worst_r, rr)
        if rr > 1:
            bad.append(f"h {h}: rows at {rr:.3f} of the bound")
        if cnt != own["count"] or [int(r[28:29].view(np.int32)[0]) for r in rows[h]] != [int((idx[h][b * 64:(b + 1) * 64] >= 0).sum()) for b in range(rows[h].shape[0])]:
            bad.append(f"h {h}: count {cnt} != {own['count']}")
        if own["count"] == 0 and acc[:27].any():
            bad.append(f"h {h}: zero valid samples but non-zero sums")
        if not step:
            continue
        # one step, teacher-forced on the kernel's own fp32 sums
        A, rhs = R.unpack_row(acc)
        st = R.step(A, rhs, cnt, T[h], R.COARSE)
        if st["x"] is None:
            if not (stopped[h, 0] == 1 and failed[h, 0] == 0 and np.array_equal(T_dev[h], T[h])):
                bad.append(f"h {h}: {cnt} valid samples must stop the hypothesis with T unchanged")
        elif failed[h, 0]:
            if not (stopped[h, 0] == 1 and np.array_equal(T_dev[h], T[h])):
                bad.append(f"h {h}: solver_failed without a stop or with T changed")
        elif st["cond"] * R.EPS >= SINGULAR:
            # numerically singular in fp32 (a first-order bound says nothing there): finite, nothing more
            if not (np.isfinite(T_dev[h]).all() and np.isfinite(x_dev[h]).all()):
                bad.append(f"h {h}: a singular system (cond {st['cond']:.2e}) gave a transform that is not finite")
        else:
            rx = float(np.abs(x_dev[h] - st["x"]).max() / R.step_bound(st["cond"], st["x"])) if np.abs(st["x"]).max() > 0 else 0.0
            worst_x = max(worst_x, rx)
            if rx > 1 or not np.isfinite(T_dev[h]).all():
                bad.append(f"h {h}: step at {rx:.3f} of the K bound (cond {st['cond']:.2e})")
    say(f"{name}: H {len(T)} M {m} O {len(observed)} threshold {threshold} huber {use_huber} excluded {n_excluded} distance {worst_d:.3f} "
        f"rows {worst_r:.3f} step {worst_x:.3f} of their bounds{'  FAIL ' + '; '.join(bad) if bad else ''}")
    return bad


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def random_surface(rng, n_tri, n):
    """n samples and unit normals on a random triangle soup"""
    tri = rng.uniform(-0.2, 0.2, (n_tri, 1, 3)) + rng.normal(0, 0.08, (n_tri, 3, 3))
    k = rng.integers(0, n_tri, n)
    w = rng.dirichlet([1, 1, 1], n)
    p = (tri[k] * w[:, :, None]).sum(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p, nrm[k]


def random_case(rng):
    h = int(rng.choice([1, 2, 3, 8]))
    m = int(rng.choice([1, 63, 64, 65, 255, 257, int(rng.integers(1, 700))]))
    o = int(rng.choice([1, 9, 63, 64, 65, 1023, 1024, 1025, int(rng.integers(1, 2500))]))
    kind = rng.choice(["plain", "plain", "coincident", "all_beyond", "few"])
    if kind == "few":
        o = int(rng.integers(1, 10))
    thr = float(rng.choice([0.01, 0.05, 0.3, np.inf]))
    p, nrm = random_surface(rng, int(rng.integers(1, 40)), m)
    truth = np.concatenate([random_rotations(rng, 1)[0], rng.uniform(-0.5, 0.5, (3, 1))], 1)
    sel = rng.integers(0, m, o)
    obs = p[sel] @ truth[:, :3].T + truth[:, 3] + rng.normal(0, 0.004, (o, 3))
    if kind == "coincident":  # as resample_points' up-sampling produces: every point several times over
        obs = obs[rng.integers(0, max(1, o // 4), o)]
    # hypotheses around the truth: small and large perturbations
    T = []
    for _ in range(h):
        d = R.update_matrix(np.concatenate([rng.normal(0, rng.choice([0.02, 0.5]), 3), rng.normal(0, 0.01, 3)]))
        T.append((d @ np.vstack([truth, [0, 0, 0, 1]]))[:3].reshape(-1))
    if kind == "all_beyond":
        obs = obs + [3.0, 0, 0]
        thr = 0.05
    return dict(mesh_points=p.astype(np.float32), mesh_normals=nrm.astype(np.float32), observed=obs.astype(np.float32),
                T=np.asarray(T, np.float32), threshold=thr, use_huber=bool(rng.integers(0, 2)), delta=float(rng.choice([0.005, 0.02])))


def main(cases, seed):
    rng = np.random.default_rng(seed)
    failed = 0
    for c in range(cases):
        failed += bool(check_case(f"case {c}", **random_case(rng)))
    print(f"fuzz_pose_icp: {cases - failed} of {cases} cases passed (seed {seed}), {failed} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]), int(sys.argv[2])))
