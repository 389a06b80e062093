"""Records tests/golden/pose_parent_bits.npz: the bits the pose estimators' launches (csrc/pose_detect.hip, csrc/pose_icp.hip)
give on fixed inputs, for tests/test_gpu_pose_parent_bits.py to hold a later build to:

    python tests/golden/make_pose_parent_bits.py            (needs the GPU; rewrites the fixture)

The float64 oracles hold these kernels inside bounds, so a changed rounding passes them; this fixture does not let it pass.
It is recorded from the build whose arithmetic is to be kept; a change that alters arithmetic on purpose re-records it with this
script and says so.  Only curobo_amd.backends.perception and backends.mesh are used.  ``inputs()`` makes every input from
fixed seeds (stored in the file under "in/..."), ``replay(inputs)`` runs the launches and returns every output word as int32
(stored under "out/..."; an output equal to an earlier one, as the per-point outputs with and without the Huber weight are, is
stored once: "same" lists such names with the earlier one's).  ``load()`` gives both back in full."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "pose_parent_bits.npz")
DEV = "cuda:0"

SDF_N = (1, 63, 64, 65, 255, 256, 257, 513)  # lane, wavefront and workgroup edges; three rows for the in-order sum
SDF_THRESHOLD, SDF_MAX_DISTANCE, SDF_DELTA = 0.05, 0.2, 0.02
LM = dict(lambda_initial=1e-3, lambda_factor=3.0, lambda_min=1e-7, lambda_max=1e4, rho_min=0.25, minimum_valid_count=10)
ICP_SHAPES = ((1, 1, 1), (63, 5, 2), (64, 64, 1), (65, 257, 3), (257, 1025, 2))  # (M, O, H)
ICP_THRESHOLD, ICP_DELTA = 0.03, 0.01
#: (use_huber, finite threshold, the last hypothesis stopped, honour_stopped)
ICP_VARIANTS = ((1, 1, 0, 1), (0, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (1, 1, 1, 1), (1, 1, 1, 0))


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]), np.array([w, x, y, z])


def _row(A, rhs, scalar, count):
    """one workspace row: the upper triangle of A, rhs, the scalar of word 27, the count"""
    row = np.zeros(32, np.float32)
    row[:21], row[21:27], row[27] = np.asarray(A)[np.triu_indices(6)], rhs, scalar
    row[28:29] = np.asarray([count], np.int32).view(np.float32)
    return row


def inputs():
    f32 = np.float32
    rng = np.random.default_rng(20261018)
    d = {}
    # ---- SDF: a tetrahedron at a general pose; points 1 mm .. 2.5 thresholds off its faces, so that some are beyond it
    V = np.array([[0.2, 0.0, -0.1], [-0.1, 0.17, -0.1], [-0.1, -0.17, -0.1], [0.0, 0.0, 0.22]])
    F = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)
    n = max(SDF_N)
    base = (V[F[rng.integers(0, 4, n)]] * rng.dirichlet([1, 1, 1], n)[:, :, None]).sum(1)
    off = rng.normal(size=(n, 3))
    pm = base + off / np.linalg.norm(off, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(1e-3), np.log(2.5 * SDF_THRESHOLD), n))[:, None]
    Rm, q = _rotation(rng)
    t = np.array([0.31, -0.12, 0.45])
    d.update(sdf_vertices=V.astype(f32), sdf_faces=F, sdf_points=(pm @ Rm.T + t).astype(f32), sdf_position=t.astype(f32), sdf_quaternion=q.astype(f32))
    # ---- LM step on one-row workspaces: a state to update from, and the rows
    J = rng.normal(0, 1, (40, 6)) * [1, 1, 1, 0.3, 0.3, 0.3]
    r = rng.normal(0, 0.01, 40)
    A, g = (J.T @ J).astype(f32), (J.T @ r).astype(f32)
    J2 = J + rng.normal(0, 0.05, J.shape)
    A2, g2 = (J2.T @ J2).astype(f32), (J2.T @ (0.8 * r)).astype(f32)
    d.update(lm_best_position=t.astype(f32), lm_best_quaternion=q.astype(f32), lm_best_JtJ=A.reshape(-1), lm_best_Jtr=g,
             lm_best=np.array([np.sqrt(r @ r / 40), r @ r, 1e-3, 0.5 * (r @ r)], f32))  # best_error, best_sum_sq, lambda_damping, pred_reduction
    ssq = f32(0.64 * (r @ r))
    inf_row, nan_row = _row(A2, g2, ssq, 40), _row(A2, g2, ssq, 40)
    inf_row[0], nan_row[7] = np.inf, np.nan
    d["lm_rows"] = np.stack([_row(A2, g2, ssq, 40), _row(-A2, g2, ssq, 40), inf_row, nan_row, _row(A2, g2, ssq, 10), _row(A2, g2, ssq, 11)])
    # ---- ICP: samples of a triangle soup, observations of it at a pose, hypotheses around that pose
    for m, o, h in ICP_SHAPES:
        tri = rng.uniform(-0.2, 0.2, (12, 1, 3)) + rng.normal(0, 0.08, (12, 3, 3))
        k = rng.integers(0, 12, m)
        p = (tri[k] * rng.dirichlet([1, 1, 1], m)[:, :, None]).sum(1)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True))[k]
        Rt, _ = _rotation(rng)
        obs = p[rng.integers(0, m, o)] @ Rt.T + t + rng.normal(0, 0.004, (o, 3))
        T = []
        for _ in range(h):
            Rd, _ = _rotation(rng)
            Rd = np.eye(3) + 0.03 * (Rd - Rd.T)  # a small turn (not orthonormal to the last bit, as a running T is not)
            T.append(np.concatenate([Rd @ Rt, (Rd @ t + rng.normal(0, 0.005, 3))[:, None]], 1).reshape(-1))
        key = f"icp_{m}_{o}_{h}"
        d.update({f"{key}_points": p.astype(f32), f"{key}_normals": nrm.astype(f32), f"{key}_observed": obs.astype(f32), f"{key}_T": np.asarray(T, f32)})
    # ---- ICP step on one-row workspaces, one hypothesis per row
    Ji = np.concatenate([rng.normal(0, 0.3, (60, 3)), rng.normal(0, 1, (60, 3))], 1)
    Ai = (Ji.T @ Ji).astype(f32)
    x = np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.005, 3)])
    bi = (Ai.astype(np.float64) @ x).astype(f32)
    small = (Ai.astype(np.float64) @ (x * (0.5e-4 / np.linalg.norm(x[3:])))).astype(f32)
    inf_row = _row(Ai, bi, 0.7, 60)
    inf_row[0] = np.inf
    d["icp_rows"] = np.stack([_row(Ai, bi, 0.7, 9), _row(Ai, bi, 0.7, 10), _row(-Ai, bi, 0.7, 60), inf_row, _row(Ai, small, 0.7, 60)])
    d["icp_rows_T"] = np.tile(np.concatenate([Rt, t[:, None]], 1).reshape(-1).astype(f32), (5, 1))
    return d


def replay(d):
    """every launch on the inputs ``d`` -> {name: int32 array}"""
    from curobo_amd.backends import perception as P
    from curobo_amd.backends.mesh import build_mesh_bvh

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()  # noqa: E731
    bits = lambda t: t.cpu().numpy().view(np.int32).copy()  # noqa: E731
    out = {}
    # ---- SDF evaluate
    mesh = build_mesh_bvh(d["sdf_vertices"], d["sdf_faces"], DEV, cells=False)
    position, quaternion = dev(d["sdf_position"]), dev(d["sdf_quaternion"])

    def evaluate(points, position, quaternion, huber):
        n = len(points)
        ws = torch.full((P.pose_sdf_ws_bytes(n) // 4,), float("nan"), device=DEV)
        dist, grad = torch.full((n,), -1.0, device=DEV), torch.full((n, 3), -1.0, device=DEV)
        valid = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        P.pose_sdf_evaluate(ws, points, position, quaternion, mesh.struct, SDF_MAX_DISTANCE, SDF_THRESHOLD, huber, SDF_DELTA, dist, grad, valid)
        return ws, (dist, grad, valid)

    for n in SDF_N:
        for huber in (0, 1):
            ws, per_point = evaluate(dev(d["sdf_points"][:n]), position, quaternion, huber)
            for name, t in zip(("ws", "distance", "gradient", "valid"), (ws, *per_point)):
                out[f"sdf_{n}_{huber}_{name}"] = bits(t)
    ws, per_point = evaluate(dev(d["sdf_points"][:65] + np.float32([2.0, 0, 0])), position, quaternion, 1)  # no valid point
    for name, t in zip(("ws", "distance", "gradient", "valid"), (ws, *per_point)):
        out[f"sdf_none_{name}"] = bits(t)
    # ---- LM: INIT and two UPDATEs on the N = 257 case, each on an evaluation at the state's candidate pose
    lm = lambda state, ws, n, mode: P.pose_lm_step(state, ws, n, mode, **LM)  # noqa: E731
    points = dev(d["sdf_points"][:257])
    state = torch.zeros(P.POSE_STATE_WORDS, device=DEV)
    state[P.pose_state_slice("cand_position")] = position
    state[P.pose_state_slice("cand_quaternion")] = quaternion
    for k, mode in enumerate((P.POSE_LM_INIT, P.POSE_LM_UPDATE, P.POSE_LM_UPDATE)):
        ws, _ = evaluate(points, state[P.pose_state_slice("cand_position")], state[P.pose_state_slice("cand_quaternion")], 1)
        lm(state, ws, 257, mode)
        out[f"lm_257_state_{k}"] = bits(state)
    # ---- LM on the one-row workspaces, both modes
    start = np.zeros(P.POSE_STATE_WORDS, np.float32)
    for f in ("best_position", "best_quaternion", "best_JtJ", "best_Jtr"):
        start[P.pose_state_slice(f)] = d[f"lm_{f}"]
    for f, v in zip(("best_error", "best_sum_sq", "lambda_damping", "pred_reduction"), d["lm_best"]):
        start[P.pose_state_slice(f)] = v
    start[P.pose_state_slice("best_n_valid")] = np.asarray([40], np.int32).view(np.float32)
    start[P.pose_state_slice("cand_position")] = d["lm_best_position"] + np.float32(0.001)
    start[P.pose_state_slice("cand_quaternion")] = d["lm_best_quaternion"]
    for k, row in enumerate(d["lm_rows"]):
        for mode in (P.POSE_LM_INIT, P.POSE_LM_UPDATE):
            state = dev(start)
            lm(state, dev(row), 1, mode)
            out[f"lm_row_{k}_{mode}"] = bits(state)
    # ---- ICP correspond, and the three steps on its workspace
    for m, o, h in ICP_SHAPES:
        key = f"icp_{m}_{o}_{h}"
        points, normals, observed = dev(d[f"{key}_points"]), dev(d[f"{key}_normals"]), dev(d[f"{key}_observed"])
        for huber, finite, stop, honour in ICP_VARIANTS:
            st = np.zeros((h, P.POSE_ICP_STATE_WORDS), np.float32)
            st[:, P.pose_icp_state_slice("T")] = d[f"{key}_T"]
            if stop:
                st[h - 1, P.pose_icp_state_slice("stopped")] = np.asarray([1], np.int32).view(np.float32)
            state = dev(st)
            ws = torch.full((P.pose_icp_ws_bytes(h, m) // 4,), 7.0, device=DEV)
            index, dist = torch.full((h, m), -7, dtype=torch.int32, device=DEV), torch.full((h, m), -1.0, device=DEV)
            P.pose_icp_correspond(ws, points, normals, observed, state, ICP_THRESHOLD if finite else float("inf"), huber, ICP_DELTA,
                                  honour_stopped=bool(honour), out_index=index, out_distance=dist)
            tag = f"{key}_{huber}{finite}{stop}{honour}"
            out[f"{tag}_ws"], out[f"{tag}_index"], out[f"{tag}_distance"] = bits(ws), bits(index), bits(dist)
            for mode in (P.POSE_ICP_COARSE, P.POSE_ICP_FINE, P.POSE_ICP_FINALIZE):
                after = state.clone()
                P.pose_icp_step(after, ws, m, mode)
                out[f"{tag}_state_{mode}"] = bits(after)
    # ---- ICP step on the one-row workspaces: one hypothesis per row
    st = np.zeros((len(d["icp_rows"]), P.POSE_ICP_STATE_WORDS), np.float32)
    st[:, P.pose_icp_state_slice("T")] = d["icp_rows_T"]
    for mode in (P.POSE_ICP_COARSE, P.POSE_ICP_FINE, P.POSE_ICP_FINALIZE):
        state = dev(st)
        P.pose_icp_step(state, dev(d["icp_rows"].reshape(-1)), 1, mode)
        out[f"icp_rows_state_{mode}"] = bits(state)
    torch.cuda.synchronize()
    return out


def pack(given, recorded):
    """the arrays of the file"""
    arrays, first, same = {f"in/{k}": v for k, v in given.items()}, {}, []
    for k, v in recorded.items():
        earlier = first.setdefault((v.shape, v.tobytes()), k)
        if earlier == k:
            arrays[f"out/{k}"] = v
        else:
            same.append((k, earlier))
    return dict(arrays, same=np.array(same))


def load(path=PATH):
    """(inputs, recorded outputs) of the file"""
    z = np.load(path)
    out = {k[4:]: z[k] for k in z.files if k.startswith("out/")}
    out.update({str(k): out[str(earlier)] for k, earlier in z["same"]})
    return {k[3:]: z[k] for k in z.files if k.startswith("in/")}, out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    given = inputs()
    recorded = replay(given)
    target = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(target, **pack(given, recorded))
    print(f"{target}: {len(given)} inputs, {len(recorded)} outputs, {sum(v.size for v in recorded.values())} words, {os.path.getsize(target)} bytes")
