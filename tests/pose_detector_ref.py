"""Float64 oracle of the mesh-SDF pose refinement (csrc/pose_detect.hip; reference wp_mesh_sdf_alignment.py, optim_pose_lm.py,
sdf_pose_detector.py): the evaluation by brute force over the triangles, one LM iteration, the bounds the tests hold fp32
results to, and the EXCLUDED SET -- the only points a test may skip:
  * points whose float64 distance is within 1e-6 m of distance_threshold, or within 1e-6 m of 1e-8;
  * points whose two nearest DISTINCT closest points differ by less than 1e-6 m in distance but by more than 1e-5 m in
    position (the medial axis: the gradient is ambiguous there).
Shared by tests/test_oracle_pose_detector.py (the reference's recorded fp32 output against this), tests/test_gpu_pose_detector.py
and tests/randomised/fuzz_pose_detector.py (the HIP kernels against this)."""

import numpy as np
from pose_rows import EPS  # noqa: F401  (shared with the ICP detector's oracle)

BAND = 1e-6
#: C of the per-point bounds (docs/ORACLE_PINS.md): distance within C 2^-24 S, gradient within 2 C 2^-24 S / dist + 4 2^-24.
#: The reference's own fp32 output on the golden cases needs 372.7 (case lsolid_n257: the gradient of a point 2.3 mm from an
#: edge of the solid under the general pose turns by 1.7e-3; its distance needs 2.6): the smallest power of two is 512; doubled.
POSE_DISTANCE_C = 1024.0
#: K of the LM step bound |delta - oracle|_inf <= K cond(J^T J + lambda I) 2^-24 |oracle|_inf.  The reference's own fp32
#: step (LAPACK on the CPU) on every recorded iteration needs 3.44 (seq_noisy): the smallest power of two is 4; doubled.
POSE_LM_K = 8.0
MINIMUM_VALID_COUNT = 10


def quat_rotate(q_wxyz, v):
    """Warp's quat_rotate (no normalisation): v (2 w^2 - 1) + 2 u (u . v) + 2 w (u x v)"""
    q = np.asarray(q_wxyz, np.float64)
    w, u = q[0], q[1:]
    v = np.asarray(v, np.float64)
    return v * (2.0 * w * w - 1.0) + 2.0 * u * (v @ u)[..., None] + 2.0 * w * np.cross(np.broadcast_to(u, v.shape), v)


def closest_on_triangles(P, A, B, C):
    """closest point of every triangle (A, B, C [T, 3]) to every point P [N, 3] -> [N, T, 3] (Ericson 5.1.5), float64"""
    P = P[:, None, :]
    ab, ac = (B - A)[None], (C - A)[None]
    ap = P - A[None]
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = P - B[None]
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = P - C[None]
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ca = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        v_in, w_in = vb * den, vc * den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    v = np.select(conds, [zero, one, v_ab, zero, zero, 1.0 - w_bc], v_in)
    w = np.select(conds, [zero, zero, zero, one, w_ca, w_bc], w_in)
    out = A[None] + v[..., None] * ab + w[..., None] * ac
    bad = ~np.isfinite(out).all(-1)  # a degenerate triangle: its first vertex
    out[bad] = np.broadcast_to(A[None], out.shape)[bad]
    return out


def evaluate(points, position, quaternion, vertices, faces, max_distance, distance_threshold, use_huber, huber_delta, chunk=512):
    """the evaluation in float64.  Returns a dict: dist, grad (world), valid, J [N, 6], r, excluded, S (per point), and the sums
    JtJ [6, 6], Jtr [6], sum_sq, n over the valid set."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    t, q = np.asarray(position, np.float64), np.asarray(quaternion, np.float64)
    V, F = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    qi = q * np.array([1.0, -1.0, -1.0, -1.0])
    pm = quat_rotate(qi, P - t)
    N = P.shape[0]
    dist, cpb, amb = np.zeros(N), np.zeros((N, 3)), np.zeros(N, bool)
    for s in range(0, N, chunk):
        cps = closest_on_triangles(pm[s:s + chunk], A, B, C)
        d = np.linalg.norm(cps - pm[s:s + chunk, None, :], axis=-1)
        k = d.argmin(1)
        rows = np.arange(d.shape[0])
        dist[s:s + chunk], cpb[s:s + chunk] = d[rows, k], cps[rows, k]
        near = d - d[rows, k][:, None] < BAND
        apart = np.linalg.norm(cps - cps[rows, k][:, None, :], axis=-1) > 1e-5
        amb[s:s + chunk] = (near & apart).any(1)
    found = dist < max_distance
    valid = found & (dist <= distance_threshold) & (dist > 1e-8)
    excluded = amb | (np.abs(dist - distance_threshold) < BAND) | (np.abs(dist - 1e-8) < BAND) | (np.abs(dist - max_distance) < BAND)
    with np.errstate(divide="ignore", invalid="ignore"):
        gm = (cpb - pm) / dist[:, None]
    gw = np.where(valid[:, None], quat_rotate(q, np.nan_to_num(gm)), 0.0)
    r = np.where(valid, dist, 0.0)
    hs = np.ones(N)
    if use_huber:
        with np.errstate(divide="ignore", invalid="ignore"):
            hs = np.where(r > huber_delta, np.sqrt(huber_delta / np.where(r > 0, r, 1.0)), 1.0)
        r = r * hs
    J = np.concatenate([gw, np.stack([gw[:, 2] * P[:, 1] - gw[:, 1] * P[:, 2], gw[:, 0] * P[:, 2] - gw[:, 2] * P[:, 0],
                                      gw[:, 1] * P[:, 0] - gw[:, 0] * P[:, 1]], 1)], 1) * hs[:, None]
    J = np.where(valid[:, None], J, 0.0)
    S = np.maximum(np.abs(pm).max(1), np.abs(V[F.reshape(-1)]).max())
    out = dict(dist=np.where(valid, dist, 0.0), raw_dist=dist, grad=gw, valid=valid, J=J, r=r, excluded=excluded, S=S, p_mesh=pm)
    out.update(sums_of(J, r, valid))
    return out


def sums_of(J, r, valid):
    """float64 sums over a valid set, and the sum of |term| per entry (for the order-free bound (N + 8) 2^-24 sum |term|)"""
    J = np.where(np.asarray(valid, bool)[:, None], np.asarray(J, np.float64), 0.0)
    r = np.where(np.asarray(valid, bool), np.asarray(r, np.float64), 0.0)
    return dict(JtJ=J.T @ J, Jtr=J.T @ r, sum_sq=float(r @ r), n=int(np.asarray(valid, bool).sum()),
                abs_JtJ=np.abs(J).T @ np.abs(J), abs_Jtr=np.abs(J).T @ np.abs(r), abs_sum_sq=float(r @ r))


def jacobian_from_outputs(points, dist, grad, valid, use_huber, huber_delta):
    """the Jacobian rows and residuals that follow from per-point fp32 outputs (distance, world gradient, valid), in float64:
    what a reduction of exactly those outputs must sum"""
    P, g = np.asarray(points, np.float64), np.asarray(grad, np.float64)
    v = np.asarray(valid).astype(bool)
    r = np.asarray(dist, np.float64).copy()
    hs = np.ones(len(r))
    if use_huber:
        big = r > np.float64(np.float32(huber_delta))
        hs[big] = np.sqrt(np.float64(np.float32(huber_delta)) / r[big])
        r = r * hs
    J = np.concatenate([g, np.stack([g[:, 2] * P[:, 1] - g[:, 1] * P[:, 2], g[:, 0] * P[:, 2] - g[:, 2] * P[:, 0],
                                     g[:, 1] * P[:, 0] - g[:, 0] * P[:, 1]], 1)], 1) * hs[:, None]
    return np.where(v[:, None], J, 0.0), np.where(v, r, 0.0), v


def point_bounds(ev, C=POSE_DISTANCE_C):
    """(distance bound [N], gradient bound [N]) of the per-point comparison"""
    tol_d = C * EPS * ev["S"]
    with np.errstate(divide="ignore"):
        tol_g = 2.0 * C * EPS * ev["S"] / np.maximum(ev["raw_dist"], 1e-300) + 4.0 * EPS
    return tol_d, tol_g


# ------------------------------------------------------------------------------------------------------------ LM
def euler_xyz_to_quat(e):
    h = np.asarray(e, np.float64) * 0.5
    cx, cy, cz, sx, sy, sz = np.cos(h[0]), np.cos(h[1]), np.cos(h[2]), np.sin(h[0]), np.sin(h[1]), np.sin(h[2])
    return np.array([cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz, cx * cy * sz - sx * sy * cz])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def pose_rotate(q, v):
    """rotation of v by the quaternion q as Pose.multiply applies it (v + w t + u x t, t = 2 u x v)"""
    w, u = q[0], np.asarray(q[1:], np.float64)
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def lm_candidate(JtJ, Jtr, lam, best_position, best_quaternion):
    """solve_lm_step, compute_predicted_reduction and the candidate pose from a best state, float64.  Returns delta, pred,
    candidate position / quaternion, cond(A), and ok = the factorisation exists."""
    A = np.asarray(JtJ, np.float64) + float(lam) * np.eye(6)
    g = np.asarray(Jtr, np.float64)
    cond = float(np.linalg.cond(A))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        nan = np.full(6, np.nan)
        return dict(delta=nan, pred=np.nan, position=nan[:3], quaternion=np.full(4, np.nan), cond=cond, ok=False)
    delta = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    pred = -(delta @ g) - 0.5 * (delta @ (np.asarray(JtJ, np.float64) @ delta))
    qd = euler_xyz_to_quat(delta[3:])
    pos = delta[:3] + pose_rotate(qd, np.asarray(best_position, np.float64))
    return dict(delta=delta, pred=float(pred), position=pos, quaternion=quat_mul(qd, np.asarray(best_quaternion, np.float64)), cond=cond,
                ok=True)


def trust_update(best_sum_sq, pred, lam, cand_sum_sq, cand_n, lambda_factor, lambda_min, lambda_max):
    """trust_region_update: (accepted, new lambda, trust ratio, candidate error).  The ratio in float64; lambda in the fp32
    arithmetic the reference defines it by (a quotient or product of two floats, clamped), so that it can be compared exactly."""
    enough = int(cand_n) > MINIMUM_VALID_COUNT
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.float64(best_sum_sq) - np.float64(cand_sum_sq)) / (np.float64(pred) + 1e-8)
    accepted = bool(ratio >= 0) and enough
    f32 = np.float32
    new = f32(lam) / f32(lambda_factor) if accepted else f32(lam) * f32(lambda_factor)
    new = f32(min(max(new, f32(lambda_min)), f32(lambda_max)))
    err = np.sqrt(np.float64(cand_sum_sq) / (np.float64(cand_n) + 1e-8)) if enough else np.inf
    return accepted, float(new), float(ratio), float(err)


def lm_step_bounds(cand, JtJ, Jtr, best_position, K=POSE_LM_K):
    """(delta, position, quaternion, pred) bounds of an fp32 LM step against ``cand`` (``lm_candidate``)"""
    rel = K * cand["cond"] * EPS
    d = np.abs(cand["delta"])
    tol_delta = rel * d.max() + 1e-30
    reach = 1.0 + np.abs(np.asarray(best_position, np.float64)).max()
    tol_pos = 2.0 * tol_delta * reach + 16.0 * EPS * reach
    tol_quat = tol_delta + 16.0 * EPS
    mag = d @ np.abs(np.asarray(Jtr, np.float64)) + d @ (np.abs(np.asarray(JtJ, np.float64)) @ d)
    tol_pred = mag * (16.0 * EPS + 2.0 * rel) + 1e-30
    return tol_delta, tol_pos, tol_quat, tol_pred
