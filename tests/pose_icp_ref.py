"""Float64 oracle of the point-to-plane ICP (csrc/pose_icp.hip; reference pose_detector.py :172-375, util.py :88-113 and
:245-330): one correspondence search by brute force, one step, the bounds the tests hold fp32 results to, and the EXCLUDED
SET -- the only samples a test may skip:
  * samples whose two nearest observed points AT DISTINCT POSITIONS differ by less than 1e-6 m in distance (fp32 may pick
    either); exact duplicates of an observed point are not excluded: the lowest index is required;
  * samples whose nearest distance is within 1e-6 m of the threshold.
Shared by tests/test_oracle_pose_icp.py (the reference's recorded fp32 sums and steps against this),
tests/test_gpu_pose_icp.py and tests/randomised/fuzz_pose_icp.py (the HIP kernels against this).

The bounds (docs/ORACLE_PINS.md).
  distance  A sample s = R p + t and an observed point o, every coordinate at most S in magnitude (S taken over |R||p| + |t|
            and |o|): s carries at most 4 roundings of size 2^-24 S per coordinate, the differences one more, so |o - s| is
            off by at most sqrt(3) 5 2^-24 S < 9 2^-24 S, and the squares, their sum and the root add 4 roundings relative to
            the distance itself: DISTANCE_BOUND = 2^-24 (9 S + 4 d).  Doubled for the fused multiply-adds' freedom: 18 S + 8 d.
  rows      A sum of N fp32 terms, in any order, is within N 2^-24 sum|term| of the exact sum of the rounded terms, and a term
            computed in fp32 is within a few 2^-24 of its own magnitude.  |term| is the product of the MAGNITUDES of its factors
            before any cancellation: |s| <= |R||p| + |t|, |n'| <= |R||n|, |s x n'|, |(o - s) . n'| and |o - s| with every product
            and coordinate taken absolute, and a Huber weight d/(|b| + 1e-10) is as uncertain as b is, relative to |b|.  The reference's recorded
            sums are held to (N + 8) 2^-24 sum|term|, as for the LM detector.  The kernel's rows are compared with the float64
            sums over ITS OWN correspondences, term for term, and a term there passes through up to 24 roundings (4 + 1 for s, 3
            for n', 3 per cross product, 6 for b, 2 for the weight, 2 for the product, twice over for J J^T): (N + 24).
  step      |x - oracle|_inf <= K cond(J^T J + 1e-6 I) 2^-24 |oracle|_inf, K = POSE_ICP_K below.
"""

import numpy as np
from pose_rows import EPS, row_bound, unpack_row  # noqa: F401  (the row's rules, shared with the LM detector's oracle)

BAND = 1e-6
DAMPING = 1e-6
MINIMUM_VALID_COUNT = 10
FINE_TRANSLATION_STOP = 1e-4
ROW_ROUNDINGS_REFERENCE = 8
ROW_ROUNDINGS_KERNEL = 24
#: K of the step bound.  MEASURED: the largest value the reference's own fp32 step (torch's cholesky_ex / cholesky_solve on the
#: CPU) needs over every recorded iteration of tests/golden/pose_icp_golden.npz, rounded up to a power of two and doubled
#: (tests/test_oracle_pose_icp.py prints the measurement and holds it under half of this): it needs 0.3545 (coarse stage), the
#: smallest power of two is 0.5; doubled.
POSE_ICP_K = 1.0
COARSE, FINE, FINALIZE = 0, 1, 2


def as_T(T):
    """[12], [3, 4] or [4, 4] -> float64 [3, 4]"""
    T = np.asarray(T, np.float64)
    return T.reshape(-1)[:12].reshape(3, 4)


def correspond(mesh_points, mesh_normals, observed, T, distance_threshold=np.inf, use_huber=True, huber_delta=0.02, index=None):
    """One hypothesis.  ``index`` None: the nearest observed point by brute force (lowest index among exact ties) and the
    excluded set; ``index`` [M] (-1 = invalid): the sums over THOSE correspondences.  Returns a dict: nearest [M], dist [M],
    index [M] (-1 beyond the threshold), excluded [M], scale, and the sums ``row`` [28] (21 upper-triangle entries of sum w J J^T,
    6 of sum w J b, sum of nearest distances), ``row_abs`` [28] (sum of term magnitudes), ``count``."""
    T = as_T(T)
    R, t = T[:, :3], T[:, 3]
    p, n, o = np.asarray(mesh_points, np.float64), np.asarray(mesh_normals, np.float64), np.asarray(observed, np.float64)
    s, nr = p @ R.T + t, n @ R.T
    s_mag, n_mag = np.abs(p) @ np.abs(R).T + np.abs(t), np.abs(n) @ np.abs(R).T
    out = {"scale": float(max(s_mag.max(), np.abs(o).max()))}
    d = np.linalg.norm(s[:, None, :] - o[None, :, :], axis=-1)  # [M, O]
    if index is None:
        nearest = d.argmin(1)  # (the first of equal minima)
        dist = d[np.arange(len(p)), nearest]
        # the runner-up at a distinct position
        same = (o[None, :, :] == o[nearest][:, None, :]).all(-1)
        other = np.where(same, np.inf, d).min(1)
        excluded = (other - dist) < BAND
        valid = dist <= distance_threshold
        if np.isfinite(distance_threshold):
            excluded |= np.abs(dist - distance_threshold) < BAND
        index = np.where(valid, nearest, -1)
        out.update(nearest=nearest, excluded=excluded)
    else:
        index = np.asarray(index).astype(np.int64)
        valid = index >= 0
        dist = d.min(1)
    out.update(dist=dist, index=index, count=int(valid.sum()))
    oc = o[np.where(valid, index, 0)]
    b = ((oc - s) * nr).sum(1)
    b_mag = ((np.abs(oc) + s_mag) * n_mag).sum(1)
    w = np.ones(len(p))
    w_mag = np.ones(len(p))
    if use_huber:
        lin = ~(np.abs(b) < huber_delta)
        w = np.where(lin, huber_delta / (np.abs(b) + 1e-10), 1.0)
        w_mag = np.where(lin, w * np.maximum(1.0, b_mag / np.maximum(np.abs(b), 1e-300)), 1.0)
    J = np.concatenate([np.cross(s, nr), nr], 1)
    c_mag = np.stack([s_mag[:, 1] * n_mag[:, 2] + s_mag[:, 2] * n_mag[:, 1], s_mag[:, 2] * n_mag[:, 0] + s_mag[:, 0] * n_mag[:, 2],
                      s_mag[:, 0] * n_mag[:, 1] + s_mag[:, 1] * n_mag[:, 0]], 1)
    J_mag = np.concatenate([c_mag, n_mag], 1)
    w, w_mag = w * valid, w_mag * valid
    iu = np.triu_indices(6)
    JtJ = (w[:, None, None] * J[:, :, None] * J[:, None, :]).sum(0)
    JtJ_mag = (w_mag[:, None, None] * J_mag[:, :, None] * J_mag[:, None, :]).sum(0)
    out["row"] = np.concatenate([JtJ[iu], (w * b) @ J, [dist.sum()]])
    # (a distance is a difference of coordinates: its magnitude before the cancellation is that of |o| + |s|)
    dist_mag = np.linalg.norm(np.abs(o[d.argmin(1)]) + s_mag, axis=1)
    out["row_abs"] = np.concatenate([JtJ_mag[iu], (w_mag * b_mag) @ J_mag, [dist_mag.sum()]])
    out["JtJ"], out["Jtb"] = JtJ, (w * b) @ J
    return out


def distance_bound(scale, dist):
    return EPS * (18.0 * scale + 8.0 * np.asarray(dist))


def solve(JtJ, Jtb):
    """(x, cond) of (J^T J + 1e-6 I) x = J^T b"""
    A = np.asarray(JtJ, np.float64) + DAMPING * np.eye(6)
    return np.linalg.solve(A, np.asarray(Jtb, np.float64)), float(np.linalg.cond(A))


def update_matrix(x):
    """T_update [4, 4] of x = (omega, t): omega_to_quaternion (util.py:49-66), then the quaternion's matrix"""
    x = np.asarray(x, np.float64)
    theta = np.linalg.norm(x[:3])
    w = np.cos(0.5 * theta)
    qx, qy, qz = x[:3] * (np.sin(0.5 * theta) / max(theta, 1e-10))
    U = np.eye(4)
    U[:3, :3] = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * w), 2 * (qx * qz + qy * w)],
                 [2 * (qx * qy + qz * w), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * w)],
                 [2 * (qx * qz - qy * w), 2 * (qy * qz + qx * w), 1 - 2 * (qx * qx + qy * qy)]]
    U[:3, 3] = x[3:]
    return U


def step(JtJ, Jtb, count, T, mode):
    """One step of one running hypothesis -> dict(x, cond, T [3, 4], stopped).  x is None when fewer than 10 samples are valid."""
    T4 = np.eye(4)
    T4[:3] = as_T(T)
    if count < MINIMUM_VALID_COUNT:
        return dict(x=None, cond=None, T=T4[:3], stopped=True)
    x, cond = solve(JtJ, Jtb)
    if mode == FINE and np.linalg.norm(x[3:]) < FINE_TRANSLATION_STOP:
        return dict(x=x, cond=cond, T=T4[:3], stopped=True)
    return dict(x=x, cond=cond, T=(update_matrix(x) @ T4)[:3], stopped=False)


def step_bound(cond, x, K=None):
    return (POSE_ICP_K if K is None else K) * cond * EPS * float(np.abs(x).max())


def pose_error(T, T_true):
    """(translation error in m, rotation error in rad) between two transforms"""
    A, Bm = as_T(T), as_T(T_true)
    Rd = A[:, :3] @ Bm[:, :3].T
    ang = np.arctan2(np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2.0, (np.trace(Rd) - 1.0) / 2.0)
    return float(np.linalg.norm(A[:, 3] - Bm[:, 3])), float(abs(ang))
