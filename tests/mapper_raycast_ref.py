"""NumPy restatement of the mapper's ray launches (curobo_amd/csrc/mapper_raycast.hip) over the arrays tests/mapper_ref.py uses,
with the reference's file:line next to each rule (paths under curobo/_src/perception/mapper/).  Every function takes ``dtype``:
np.float64 is the oracle the device is held to, np.float32 the same statement in the device's precision -- the gap between the
two is what rounding alone can do to these algorithms, and the device's bounds are multiples of it (docs/ORACLE_PINS.md).

Where float32 and float64 may legitimately decide differently the functions say so per pixel / per sample (``ambiguous``):
  * a marched sample whose |sdf| is below SIGN_ULPS ulp of the truncation distance (the sign test of the hit);
  * a sample position so near a voxel face that the set of valid corners -- and with it whether the sample is valid at all --
    changes within FACE_TOL voxel (checked by sampling again at v +- FACE_TOL), or, in the accelerated march, so near a block
    face that the block entered, and with it the jump, changes;
  * a corner whose weight EQUALS the minimum;
  * |sdf_k0| within THRESHOLD_TOL of the distance threshold, a depth within it of the depth range, sample_t of 0.1.

Warp's own definitions, read in tests/golden/warp_emulator/warp/__init__.py: wp.sign(0) = +1 (``-1 if a < 0 else 1``);
wp.quat_rotate(q, v) = v (2 w^2 - 1) + 2 w (q_v x v) + 2 q_v (q_v . v), which is not the C-library sandwich product."""

from __future__ import annotations

import numpy as np

import mapper_ref as R
import pose_detector_ref as PR

FACE_TOL = 3e-5        # voxels: a float32 coordinate of up to 64 voxels is off by <= 4e-6, the position under it by <= 6e-6 voxel
SIGN_ULPS = 16
THRESHOLD_TOL = 1e-6   # metres
MIN_STEP_SCALE = 0.5   # builder_raycast.py:56
HIT_REFINE_ITERATIONS = 10  # :57
MAX_ITERATIONS = 10000  # :518, :754
UP = (0.0, 0.0, 1.0)


class DenseMap:
    """the TSDF as the samplers see it: per voxel of the PADDED grid the sdf, whether it is valid (inside the padded grid, block
    ever visible, weight >= minimum: builder_raycast.py:63-90) and whether its weight equals the minimum"""

    def __init__(self, g: "R.Grid", sw, w, visible, min_weight: float, dtype):
        self.g, self.dtype = g, dtype
        nbx, nby, nbz = g.nb
        bs = g.bs
        self.P = np.array([nbx * bs, nby * bs, nbz * bs])

        def dense(a):
            return a.reshape(nbz, nby, nbx, bs, bs, bs).transpose(0, 3, 1, 4, 2, 5).reshape(nbz * bs, nby * bs, nbx * bs)

        wv, sv = np.asarray(w, np.float16).astype(dtype), np.asarray(sw, np.float16).astype(dtype)
        vis = np.broadcast_to(np.asarray(visible, bool)[: g.n_blocks, None], wv.shape)
        mw = dtype(np.float32(min_weight))
        self.block_visible = np.asarray(visible, bool)[: g.n_blocks]
        self.ok = dense(vis & (wv >= mw))                                                                     # :78
        self.at_minimum = dense(vis & (wv == mw))
        with np.errstate(divide="ignore", invalid="ignore"):
            self.sdf = dense(np.where(wv > 0, sv / np.where(wv > 0, wv, 1), 0).astype(dtype))
        self.origin = np.asarray(g.origin, dtype)
        self.half = np.array([g.nx, g.ny, g.nz], dtype) * dtype(0.5)
        self.vs, self.trunc = dtype(g.vs), dtype(g.trunc)

    def continuous(self, p):
        return (p - self.origin) / self.vs + self.half                                                        # builder_coord.py:45-54

    def _trilinear_v(self, v):
        """(sdf, valid, touches a weight at the minimum) at continuous coordinates v [n, 3]  (builder_raycast.py:168-258)"""
        dt = self.dtype
        f = v - dt(0.5)
        f0 = np.floor(f)
        t = f - f0
        with np.errstate(invalid="ignore"):
            i0 = np.where(np.isfinite(f0), np.clip(f0, -4, self.P.max() + 4), -4).astype(np.int64)
        total = np.zeros(len(v), dt)
        any_valid, touch = np.zeros(len(v), bool), np.zeros(len(v), bool)
        for k in range(8):
            d = np.array([k & 1, (k >> 1) & 1, k >> 2])
            idx = i0 + d
            inside = ((idx >= 0) & (idx < self.P)).all(-1)
            c = np.clip(idx, 0, self.P - 1)
            ok = inside & self.ok[c[:, 2], c[:, 1], c[:, 0]]
            s = self.sdf[c[:, 2], c[:, 1], c[:, 0]]
            wgt = np.where(d[0], t[:, 0], dt(1) - t[:, 0]) * np.where(d[1], t[:, 1], dt(1) - t[:, 1]) * np.where(d[2], t[:, 2], dt(1) - t[:, 2])
            total = total + wgt * np.where(ok, s, self.trunc)
            any_valid |= ok
            touch |= inside & self.at_minimum[c[:, 2], c[:, 1], c[:, 0]]
        return np.where(any_valid, total, dt(R.SDF_INVALID)), any_valid, touch

    def sample(self, p):
        """(sdf, valid, ambiguous) at world positions p [n, 3]"""
        v = self.continuous(p)
        sdf, valid, touch = self._trilinear_v(v)
        f = v - self.dtype(0.5)
        amb = touch.copy()
        with np.errstate(invalid="ignore"):
            near = np.nonzero((np.abs(f - np.rint(f)) < FACE_TOL).any(-1))[0]  # only there can +-FACE_TOL change the corners
        for sgn in (-1.0, 1.0):
            if len(near):
                amb[near] |= self._trilinear_v(v[near] + self.dtype(sgn * FACE_TOL))[1] != valid[near]
        return sdf, valid, amb

    def gradient(self, p):
        """(unit gradient [n, 3], ambiguous): central difference of six trilinear samples at +-voxel_size, (0, 0, 1) where one is
        invalid or the magnitude is below 1e-6  (:277-325)"""
        dt = self.dtype
        s, amb = [], np.zeros(len(p), bool)
        bad = np.zeros(len(p), bool)
        for k in range(6):
            q = p.copy()
            q[:, k // 2] = q[:, k // 2] + (-self.vs if k & 1 else self.vs)
            sdf, valid, a = self.sample(q)
            s.append(sdf)
            bad |= ~valid
            amb |= a
        grad = np.stack([(s[0] - s[1]) / (dt(2) * self.vs), (s[2] - s[3]) / (dt(2) * self.vs), (s[4] - s[5]) / (dt(2) * self.vs)], -1)
        mag = np.sqrt((grad * grad).sum(-1))
        flat = bad | (mag < dt(1e-6))
        out = np.where(flat[:, None], np.asarray(UP, dt), grad / np.where(flat, dt(1), mag)[:, None])
        return out.astype(dt), amb


def camera_rays(K, quat, H, W, half_pixel, dtype, stride=1):
    """(world rays [n, 3], camera rays, |un-normalised ray| [n], pixel rows, pixel columns) of the pixels (i stride, j stride)"""
    K, quat = np.asarray(K, np.float32).astype(dtype), np.asarray(quat, np.float32).astype(dtype)
    pi, pj = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    pi, pj = pi.reshape(-1), pj.reshape(-1)
    off = dtype(0.5 if half_pixel else 0.0)
    rx, ry = (pj.astype(dtype) + off - K[0, 2]) / K[0, 0], (pi.astype(dtype) + off - K[1, 2]) / K[1, 1]
    ray_len = np.sqrt(rx * rx + ry * ry + dtype(1))
    ray_cam = np.stack([rx / ray_len, ry / ray_len, dtype(1) / ray_len], -1)
    return R.quat_rotate(quat, ray_cam).astype(dtype), ray_cam, ray_len, pi, pj


def _refine(M, cam, ray, t_lo, t_hi, s_lo, s_hi):
    """refine_hit_bisection  (:381-422)"""
    dt = M.dtype
    t_lo, t_hi, s_lo, s_hi = t_lo.copy(), t_hi.copy(), s_lo.copy(), s_hi.copy()
    denom = s_lo - s_hi
    small = np.abs(denom) < dt(1e-6)                                                                          # :394
    amb = np.zeros(len(denom), bool)
    t_mid = np.where(small, (t_lo + t_hi) * dt(0.5), t_lo + s_lo * (t_hi - t_lo) / np.where(small, dt(1), denom))
    live = ~small
    for _ in range(HIT_REFINE_ITERATIONS):
        if not live.any():
            break
        sdf, valid, a = M.sample(cam + ray * t_mid[:, None])
        amb |= live & a
        live = live & valid & ~(np.abs(sdf) < dt(1e-6))                                                       # :404-407
        pos = live & (sdf > 0)
        neg = live & ~(sdf > 0)
        t_lo, s_lo = np.where(pos, t_mid, t_lo), np.where(pos, sdf, s_lo)
        t_hi, s_hi = np.where(neg, t_mid, t_hi), np.where(neg, sdf, s_hi)
        denom = s_lo - s_hi
        small = np.abs(denom) < dt(1e-6)
        new = np.where(small, (t_lo + t_hi) * dt(0.5), t_lo + s_lo * (t_hi - t_lo) / np.where(small, dt(1), denom))
        t_mid = np.where(live, new, t_mid)
    return t_mid, amb


def _block_exit(M, cam, ray, b):
    """ray_block_exit_t (:424-461) for block coordinates b [n, 3] (whole numbers)"""
    dt, bs = M.dtype, M.dtype(M.g.bs)
    lo = (b * bs - M.half) * M.vs + M.origin                                                                  # builder_coord.py:68-78
    hi = (b * bs + bs - M.half) * M.vs + M.origin
    big = np.where(ray < 0, dt(-1e10), dt(1e10))                                                              # wp.sign(0) = +1
    with np.errstate(divide="ignore"):
        inv = np.where(np.abs(ray) > dt(1e-8), dt(1) / np.where(ray == 0, dt(1), ray), big)                   # :446-448
    t_far = np.maximum((lo - cam) * inv, (hi - cam) * inv)
    return t_far.min(-1)


def raycast(g, sw, w, visible, K, pos, quat, H, W, t_min, t_max, min_weight, accelerated, dtype=np.float64):
    """both forms of the raycast: raycast_block_sparse_kernel (:467-573) and raycast_block_sparse_accelerated_kernel (:690-834).
    Returns dict(points [H W, 3], normals [H W, 3], depth [H W] = range along the ray, mask bool, ambiguous bool, ray_cam_z)."""
    dt = dtype
    M = DenseMap(g, sw, w, visible, min_weight, dt)
    cam = np.asarray(pos, np.float32).astype(dt)
    ray, ray_cam, _, _, _ = camera_rays(K, quat, H, W, True, dt)
    n = H * W
    t_min, t_max = dt(np.float32(t_min)), dt(np.float32(t_max))
    step = M.vs * dt(MIN_STEP_SCALE)                                                                          # :516
    n_iter = MAX_ITERATIONS if accelerated else min(int((t_max - t_min) / step) + 1, MAX_ITERATIONS)           # :517-518, :754
    t, prev_sdf, prev_t = np.full(n, t_min, dt), np.full(n, 1e10, dt), np.full(n, t_min, dt)
    hit, done, amb = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    hit_lo, hit_s = np.zeros(n, dt), np.zeros(n, dt)
    cur = np.full((n, 3), -999999.0, dt)
    allocated, exit_t = np.zeros(n, bool), np.zeros(n, dt)
    nb = np.array(g.nb)
    for _ in range(n_iter):
        done |= ~(t <= t_max)                                                                                 # :528
        a = np.nonzero(~done)[0]
        if len(a) == 0:
            break
        p = cam + ray[a] * t[a, None]                                                                         # :531
        if accelerated:
            vb = M.continuous(p) / dt(g.bs)
            b = np.floor(vb)                                                                                  # builder_coord.py:122-136
            near = (np.abs(vb - np.rint(vb)) < FACE_TOL / g.bs).any(-1)
            changed = (b != cur[a]).any(-1)                                                                   # :767
            inside = ((b >= 0) & (b < nb)).all(-1)
            bi = np.clip(np.where(np.isfinite(b), b, 0), 0, nb - 1).astype(np.int64)
            alloc = inside & M.block_visible[(bi[:, 2] * nb[1] + bi[:, 1]) * nb[0] + bi[:, 0]]                  # :772-779
            if near.any():  # the block on the other side of the face: would the march have done the same there?
                for sgn in (-1.0, 1.0):
                    b2 = np.floor(vb + sgn * FACE_TOL / g.bs)
                    in2 = ((b2 >= 0) & (b2 < nb)).all(-1)
                    bi2 = np.clip(np.where(np.isfinite(b2), b2, 0), 0, nb - 1).astype(np.int64)
                    al2 = in2 & M.block_visible[(bi2[:, 2] * nb[1] + bi2[:, 1]) * nb[0] + bi2[:, 0]]
                    amb[a] |= near & ~(alloc & al2)
            cur[a] = np.where(changed[:, None], b, cur[a])
            allocated[a] = np.where(changed, alloc, allocated[a])
            exit_t[a] = np.where(changed, _block_exit(M, cam, ray[a], b), exit_t[a])                          # :781-787
            skip = ~allocated[a]
            t[a] = np.where(skip, exit_t[a] + step, t[a])                                                     # :789-792
            prev_sdf[a] = np.where(skip, dt(1e10), prev_sdf[a])
            a, p = a[~skip], p[~skip]
            if len(a) == 0:
                continue
        sdf, valid, sa = M.sample(p)                                                                          # :533
        amb[a] |= sa | (valid & (np.abs(sdf) < SIGN_ULPS * np.spacing(np.float32(g.trunc))))
        is_hit = valid & (prev_sdf[a] < 1e9) & (prev_sdf[a] > 0) & (sdf < 0)                                    # :541
        h = a[is_hit]
        hit[h], done[h], hit_lo[h], hit_s[h] = True, True, prev_t[h], sdf[is_hit]
        adv = valid & ~is_hit
        prev_sdf[a] = np.where(adv, sdf, prev_sdf[a])                                                         # :555-557
        prev_t[a] = np.where(adv, t[a], prev_t[a])
        t[a] = np.where(is_hit, t[a], t[a] + step)                                                            # :538, :557
    out = dict(points=np.zeros((n, 3), dt), normals=np.zeros((n, 3), dt), depth=np.zeros(n, dt), mask=hit, ambiguous=amb, ray_cam_z=ray_cam[:, 2])
    h = np.nonzero(hit)[0]
    if len(h):
        hit_t, ra = _refine(M, cam, ray[h], hit_lo[h], t[h], prev_sdf[h], hit_s[h])                            # :542-551
        pts = cam + ray[h] * hit_t[:, None]                                                                   # :562
        nrm, ga = M.gradient(pts)                                                                             # :563
        out["points"][h], out["normals"][h], out["depth"][h] = pts, nrm, hit_t                                # :564: hit_t * 1.0
        amb[h] |= ra | ga
    return out


def ray_align(g, sw, w, visible, depth, K, pos, quat, stride, n_samples, depth_min, depth_max, distance_threshold, min_weight,
              dtype=np.float64):
    """_ray_sdf_alignment_block_sparse_tiled_kernel (wp_raycast_pose_refine.py:100-316) per sample, in launch order (pixel major, then
    k): dict(J [n, 6], r [n], valid [n], ambiguous [n])"""
    dt = dtype
    M = DenseMap(g, sw, w, visible, min_weight, dt)
    H, W = depth.shape
    cam = np.asarray(pos, np.float32).astype(dt)
    n = -(-H // stride) * -(-W // stride) * n_samples
    J, r = np.zeros((n, 6), dt), np.zeros(n, dt)
    valid, amb = np.zeros(n, bool), np.zeros(n, bool)
    if not (np.isfinite(np.asarray(pos, np.float64)).all() and np.isfinite(np.asarray(quat, np.float64)).all()):
        return dict(J=J, r=r, valid=valid, ambiguous=amb)
    ray, _, ray_len, pi, pj = camera_rays(K, quat, H, W, False, dt, stride)                                    # :149-152, :171-180
    d = np.asarray(depth, np.float32)[pi, pj].astype(dt)
    lo, hi, thr = dt(np.float32(depth_min)), dt(np.float32(depth_max)), dt(np.float32(distance_threshold))
    with np.errstate(invalid="ignore"):
        d_ok = np.isfinite(d) & (d >= lo) & (d <= hi)                                                         # :159
        d_amb = np.isfinite(d) & ((np.abs(d - lo) < THRESHOLD_TOL) | (np.abs(d - hi) < THRESHOLD_TOL))
    dd = np.where(d_ok, d, dt(1))
    obs_t = dd * ray_len                                                                                      # :181
    s0, v0, a0 = M.sample(cam + ray * obs_t[:, None])                                                         # :184-185
    ray_ok = d_ok & v0 & (np.abs(s0) <= thr)                                                                  # :187
    ray_amb = d_amb | (d_ok & (a0 | (v0 & (np.abs(np.abs(s0) - thr) < THRESHOLD_TOL))))
    for ki in range(n_samples):
        k = ki - n_samples // 2                                                                               # :145-146
        sample_t = obs_t + dt(k) * M.vs                                                                       # :189
        p = cam + ray * sample_t[:, None]
        sdf, sv, sa = M.sample(p)                                                                             # :193
        expected = dt(-k) * M.vs                                                                              # :196
        ok = ray_ok & (sample_t >= dt(0.1)) & sv & (abs(expected) <= M.trunc)                                 # :191, :198
        res = np.where(ok, sdf - expected, dt(0))
        abs_r, delta = np.abs(res), dt(0.05) * (sample_t * sample_t)                                          # :202-205
        big = ok & (abs_r > delta)
        hs = np.where(big, np.sqrt(delta / np.where(big, abs_r, dt(1))), dt(1))                               # :207-208
        grad, ga = M.gradient(p)                                                                              # :212
        rows = np.concatenate([grad, np.stack([grad[:, 2] * p[:, 1] - grad[:, 1] * p[:, 2], grad[:, 0] * p[:, 2] - grad[:, 2] * p[:, 0],
                                               grad[:, 1] * p[:, 0] - grad[:, 0] * p[:, 1]], -1)], -1) * hs[:, None]  # :225-230
        at = np.arange(len(d)) * n_samples + ki
        J[at], r[at], valid[at] = np.where(ok[:, None], rows, dt(0)), np.where(ok, res * hs, dt(0)), ok
        amb[at] = ray_amb | (ray_ok & ((np.abs(sample_t - 0.1) < THRESHOLD_TOL) | sa | (ok & (ga | (np.abs(abs_r - delta) < 1e-7)))))
    return dict(J=J, r=r, valid=valid, ambiguous=amb)


def align_sums(ev, keep=None):
    """the 28 sums of the workspace row (upper triangle of J^T J row major, J^T r, sum r^2) over the valid samples (and ``keep``) in
    float64, the same of the terms' magnitudes, and the count"""
    v = ev["valid"] if keep is None else ev["valid"] & keep
    J, r = np.asarray(ev["J"], np.float64)[v], np.asarray(ev["r"], np.float64)[v]
    iu = np.triu_indices(6)
    sums = np.concatenate([(J.T @ J)[iu], J.T @ r, [r @ r]])
    mags = np.concatenate([(np.abs(J).T @ np.abs(J))[iu], np.abs(J).T @ np.abs(r), [r @ r]])
    return sums, mags, int(v.sum())


def refine(g, sw, w, visible, depth, K, pos, quat, cfg, dtype=np.float64):
    """BlockSparseRaycastPoseRefiner.refine_pose (pose_refiner.py:311-631) with the sums of ``ray_align``: (position, quaternion,
    final error, initial error).  ``cfg``: the refiner's configuration (any object with its fields)."""
    H, W = depth.shape
    stride = max(1, int((H * W / cfg.n_points) ** 0.5))                                                      # :342

    def evaluate(p, q):
        ev = ray_align(g, sw, w, visible, depth, K, np.float32(p), np.float32(q), stride, cfg.n_samples_per_ray, cfg.depth_minimum_distance,
                       cfg.depth_maximum_distance, cfg.distance_threshold, cfg.minimum_tsdf_weight, dtype)
        s, _, n = align_sums(ev)
        return (*_unpack(s), float(s[27]), n)

    best_p, best_q = np.asarray(pos, np.float64), np.asarray(quat, np.float64)
    JtJ, Jtr, best_sq, best_n = evaluate(best_p, best_q)
    initial = np.sqrt(best_sq / (best_n + 1e-8)) if best_n > 0 else np.inf                                    # :406-410
    best_err, lam = initial, float(np.float32(cfg.lambda_initial))
    for _ in range(cfg.outer_iterations * cfg.inner_iterations):
        cand = PR.lm_candidate(JtJ, Jtr, lam, best_p, best_q)                                                 # :458-476
        if cand["ok"]:
            cJ, cr, c_sq, c_n = evaluate(cand["position"], cand["quaternion"])
        else:
            cJ, cr, c_sq, c_n = np.zeros((6, 6)), np.zeros(6), 0.0, 0
        enough = c_n > cfg.minimum_valid_depth_pixels                                                         # :548, optim_pose_lm.py:53-175
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (best_sq - c_sq) / (cand["pred"] + 1e-8)
        if bool(ratio >= 0) and enough:
            best_p, best_q, JtJ, Jtr, best_sq, best_n = cand["position"], cand["quaternion"], cJ, cr, c_sq, c_n
            best_err = np.sqrt(c_sq / (c_n + 1e-8))
            lam = max(lam / cfg.lambda_factor, cfg.lambda_min)
        else:
            lam = min(lam * cfg.lambda_factor, cfg.lambda_max)
    return best_p, best_q, float(best_err), float(initial)


def _unpack(s):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    return A + np.triu(A, 1).T, np.asarray(s[21:27], np.float64)


def sphere_ground_range(cam, ray):
    """exact range along unit rays to the scene of mapper_ref (a sphere of SPHERE_RADIUS at the origin over z = GROUND_Z), inf where
    the ray meets neither, and which of the two it meets (0 sphere, 1 ground)"""
    cam, ray = np.asarray(cam, np.float64), np.asarray(ray, np.float64)
    b, c = 2.0 * (ray * cam).sum(-1), (cam * cam).sum() - R.SPHERE_RADIUS ** 2
    disc = b * b - 4 * c
    t_s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / 2, np.inf)
    t_s = np.where(t_s > 0, t_s, np.inf)
    down = ray[:, 2] < -1e-9
    t_p = np.where(down, (R.GROUND_Z - cam[2]) / np.where(down, ray[:, 2], -1.0), np.inf)
    t_p = np.where(t_p > 0, t_p, np.inf)
    return np.minimum(t_s, t_p), (t_p < t_s).astype(int)
