"""NumPy restatement in float64 of the two perception launches (test infrastructure, like the rest of ``oracle/``):
``filter_depth_ref`` for ``curobo_hip_filter_depth`` and ``robot_mask_ref`` for ``curobo_hip_robot_mask``, written from the
semantics block at the top of ``curobo_amd/csrc/perception.hip``.  Pinned on the CPU by ``tests/test_oracle_perception.py`` to
the reference's recorded outputs (``tests/golden/perception_golden.npz`` and ``perception_edges_golden.npz``).

The bands (the only pixels a comparison may skip) are those of ``tests/golden/make_perception_golden.py``:
  filter  a decisive comparison within ``FILTER_BAND`` = 1e-6 m of its threshold (``filter_band_ref``)
  mask    ``|distance + threshold| < MASK_BAND`` = 1e-5 m (``mask_band_ref``)"""

import numpy as np

FILTER_BAND, MASK_BAND = 1e-6, 1e-5


# ------------------------------------------------------------------------------------------------ depth filter
def filter_band_ref(depth, dmin, dmax, enable_flying, tolerance):
    """(B, H, W) bool: the pixel or one of its 4 clamped neighbours within FILTER_BAND of a range limit, or the largest
    neighbour difference within FILTER_BAND of tolerance * depth (any H, W >= 1)"""
    d = np.asarray(depth).astype(np.float64)
    near_limit = (np.abs(d - dmin) < FILTER_BAND) | (np.abs(d - dmax) < FILTER_BAND)
    edge = ((0, 0), (1, 1), (1, 1))
    pad, pad_lim = np.pad(d, edge, mode="edge"), np.pad(near_limit, edge, mode="edge")
    cut = [np.s_[:, 1:-1, :-2], np.s_[:, 1:-1, 2:], np.s_[:, :-2, 1:-1], np.s_[:, 2:, 1:-1]]  # left, right, up, down
    band = near_limit.copy()
    if enable_flying:
        for c in cut:
            band |= pad_lim[c]
        with np.errstate(invalid="ignore"):
            diffs = [np.abs(d - np.where((pad[c] < dmin) | (pad[c] > dmax), d, pad[c])) for c in cut]
            m = np.fmax(np.fmax(diffs[0], diffs[1]), np.fmax(diffs[2], diffs[3]))
            band |= np.abs(m - np.float64(np.float32(tolerance)) * d) < FILTER_BAND
    return band


def _pick_max(a, b):
    return np.where(a > b, a, b)  # a > b ? a : b: a NaN in b wins, a NaN in a loses


def _shift(img, di, dj, fill):
    """img[:, y + di, x + dj], ``fill`` where that lies outside the image"""
    B, H, W = img.shape
    out = np.full_like(img, fill)
    ys, xs = slice(max(0, -di), min(H, H - di)), slice(max(0, -dj), min(W, W - dj))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[:, ys, xs] = img[:, ys.start + di:ys.stop + di, xs.start + dj:xs.stop + dj]
    return out


def _bilateral(img, centre_ok, ri, rj, dmin, dmax, ss2, sd2):
    """taps inside the image and not outside [dmin, dmax] (a NaN tap is not outside: it poisons the sums and the centre is
    kept); pixels where ``centre_ok`` is false give 0"""
    sum_val, sum_w = np.zeros_like(img), np.zeros_like(img)
    inside_src = np.ones(img.shape, bool)
    for di in range(-ri, ri + 1):
        for dj in range(-rj, rj + 1):
            dn, inside = _shift(img, di, dj, 0.0), _shift(inside_src, di, dj, False)
            use = inside & ~((dn < dmin) | (dn > dmax))
            w = np.exp(-float(di * di + dj * dj) / ss2) * np.exp(-((dn - img) ** 2) / sd2)
            sum_val += np.where(use, dn * w, 0.0)
            sum_w += np.where(use, w, 0.0)
    out = np.where(sum_w > 1e-8, sum_val / np.where(sum_w > 1e-8, sum_w, 1.0), img)
    return np.where(centre_ok, out, 0.0)


def filter_depth_ref(depth, dmin, dmax, enable_flying, tolerance, kernel_size, sigma_spatial_sq2, sigma_depth_sq2, with_band=False):
    """(B, H, W) depth -> (filtered float64, valid bool) [, excluded band].  ``kernel_size`` 0 / None: no smoothing; 1 .. 5 one
    fused pass; >= 7 three passes (range + flying, rows, columns).  The scalar parameters are rounded to fp32 first, as the
    launch receives them.  A rejected pixel is 0 in the result whatever the later passes made of the 0 it carried."""
    d = np.asarray(depth).astype(np.float64)
    lo, hi, tol = (np.float64(np.float32(v)) for v in (dmin, dmax, tolerance))
    ss2, sd2 = np.float64(np.float32(sigma_spatial_sq2)), np.float64(np.float32(sigma_depth_sq2))
    ksize = int(kernel_size or 0)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(d) & ~((d < lo) | (d > hi))
        if enable_flying:
            edge = ((0, 0), (1, 1), (1, 1))
            pad = np.pad(d, edge, mode="edge")
            nb = [pad[:, 1:-1, :-2], pad[:, 1:-1, 2:], pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]]  # left, right, up, down
            diff = [np.abs(d - np.where((x < lo) | (x > hi), d, x)) for x in nb]
            m = _pick_max(_pick_max(diff[0], diff[1]), _pick_max(diff[2], diff[3]))
            valid &= ~(m > tol * d)
        r = ksize // 2
        if ksize == 0:
            out = np.where(valid, d, 0.0)
        elif ksize < 7:
            out = _bilateral(d, valid, r, r, lo, hi, ss2, sd2)
        else:
            first = np.where(valid, d, 0.0)
            in_range = lambda x: ~((x < lo) | (x > hi))  # noqa: E731  (the later passes: no finite test)
            rows = _bilateral(first, in_range(first), 0, r, lo, hi, ss2, sd2)
            out = _bilateral(rows, in_range(rows), r, 0, lo, hi, ss2, sd2)
            out = np.where(valid, out, 0.0)
    if with_band:
        return out, valid, filter_band_ref(depth, dmin, dmax, enable_flying, tolerance)
    return out, valid


# ------------------------------------------------------------------------------------------------ robot mask
def round_bf16(x):
    """fp32 -> bf16 (nearest even, NaN kept) -> float64"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float64)


def robot_frame_points_ref(depth, rays, cam_position, cam_quaternion, bf16_ops):
    """(B, H W, 3) float64: depth x ray (both, and the product, rounded to bf16 in bf16-ops mode) moved by the camera pose"""
    depth = np.asarray(depth, np.float32)
    B, H, W = depth.shape
    n = H * W
    rays = np.broadcast_to(np.asarray(rays, np.float32).reshape(-1, n, 3), (B, n, 3))
    pos = np.broadcast_to(np.asarray(cam_position, np.float32).reshape(-1, 3), (B, 3)).astype(np.float64)
    quat = np.broadcast_to(np.asarray(cam_quaternion, np.float32).reshape(-1, 4), (B, 4)).astype(np.float64)
    d = depth.reshape(B, n)
    if bf16_ops:
        cam = round_bf16((round_bf16(d)[..., None] * round_bf16(rays)).astype(np.float32))  # (bf16 x bf16 is exact in fp32)
    else:
        cam = d.astype(np.float64)[..., None] * rays.astype(np.float64)
    w, u = quat[:, None, 0:1], quat[:, None, 1:4]
    return cam * (2.0 * w * w - 1.0) + 2.0 * w * np.cross(u, cam) + 2.0 * u * (u * cam).sum(-1, keepdims=True) + pos[:, None]


def robot_mask_ref(depth, rays, cam_position, cam_quaternion, spheres, threshold, bf16_ops):
    """depth (B, H, W), rays (B or 1, H W, 3), pose (B or 1, 3) / (B or 1, 4) wxyz, spheres (B or 1, S, 4) ->
    (mask bool (B, H, W), depth_out (B, H, W) in depth's dtype, distance float64 (B, H, W)); distance is
    max_s (r_s - |p - c_s|) over the spheres with r_s >= 0, -inf without one"""
    depth = np.asarray(depth, np.float32)
    B, H, W = depth.shape
    n = H * W
    d = depth.reshape(B, n)
    p = robot_frame_points_ref(depth, rays, cam_position, cam_quaternion, bf16_ops)
    spheres = np.asarray(spheres, np.float32)
    sph = np.broadcast_to(spheres.reshape(spheres.shape[0], -1, 4), (B, spheres.shape[-2], 4))
    sph = round_bf16(sph) if bf16_ops else sph.astype(np.float64)
    distance = np.full((B, n), -np.inf)
    for b in range(B):
        s = sph[b][sph[b, :, 3] >= 0]
        for s0 in range(0, len(s), 256):  # bounded memory: pixels x 256 spheres at a time
            c = s[s0:s0 + 256]
            gap = c[None, :, 3] - np.sqrt(((p[b][:, None, :] - c[None, :, :3]) ** 2).sum(-1))
            distance[b] = np.maximum(distance[b], gap.max(1))
    mask = (d > 0) & (distance > -np.float64(np.float32(threshold)))
    depth_out = np.where(mask, np.float32(0), d)
    return mask.reshape(B, H, W), depth_out.reshape(B, H, W), distance.reshape(B, H, W)


def mask_band_ref(distance, threshold):
    return np.abs(distance + np.float64(np.float32(threshold))) < MASK_BAND
