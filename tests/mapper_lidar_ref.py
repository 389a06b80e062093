"""Float64 NumPy restatement of the mapper's lidar stages (curobo_amd/csrc/mapper_lidar.hip) and of the lidar frustum of the decay
(curobo_amd/csrc/mapper.hip: block_in_frusta), with the reference's file:line next to each rule (paths under
curobo/_src/perception/mapper/kernel/builder/).  Same standing as tests/mapper_ref.py: the device is compared with THIS.

pi and 2 pi are the reference's fp32 constants (builder_lidar_integrate.py:52-53) widened, not numpy's: the launch widens the same two.

Where float32 and float64 may decide differently the functions say so instead of deciding.  Blocks are *sure* or *possible*, as in
mapper_ref.mark_blocks.  A voxel is *ambiguous* when, for some sensor that gets that far, u or v is within UV_TOL = 1e-4 px of an
integer or a half-integer (v only where the image has more than one row), its range or elevation is within BOUND_TOL = 1e-5 of a
bound, the bilinear result's largest corner difference is within GUARD_TOL = 1e-5 m of the linear guard, the distance to the
nearest pixel's ray is within GUARD_TOL of the nearest guard, or the sdf is within SDF_TOL = 1e-5 m of -truncation.  Frustum
flags are sure in, sure out, or either."""

from __future__ import annotations

import numpy as np

import mapper_ref as R

PI = float(np.float32(3.141592653589793))       # builder_lidar_integrate.py:52
TWO_PI = float(np.float32(6.283185307179586))   # :53
UV_TOL, BOUND_TOL, GUARD_TOL, SDF_TOL, ANGLE_TOL = 1e-4, 1e-5, 1e-5, 1e-5, 1e-5
SPHERE_FACTOR = float(np.float32(0.866))        # builder_decay.py:265


def f32(x) -> float:
    return float(np.float32(x))


def pixel_rays(H: int, W: int, min_elev: float, max_elev: float) -> np.ndarray:
    """[H, W, 3] unit rays in the sensor frame  (_lidar_pixel_ray, builder_lidar_integrate.py:75-94)"""
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    az = px * TWO_PI / W - PI                                                                                  # :83, no half pixel
    el = max_elev - py * (max_elev - min_elev) / (H - 1) if H > 1 else np.full_like(py, min_elev)              # :84-88
    return np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1)                        # :89-94


def _valid(value, lo, hi):
    return (value >= lo) & (value <= hi)                                                                       # _range_valid :106-112


# ---------------------------------------------------------------------------------------------------- stage 1: visible blocks
def mark_blocks(g: "R.Grid", rng, pos, quat, valid_range, elev_range):
    """(sure, possible) bool [n_blocks]  (lidar_compute_block_keys_only_kernel :114-180)"""
    rng, pos, quat, valid_range, elev_range = (np.asarray(a, np.float64) for a in (rng, pos, quat, valid_range, elev_range))
    n, H, W = rng.shape
    sure, possible = np.zeros(g.n_blocks, bool), np.zeros(g.n_blocks, bool)
    dims = np.array([g.nx, g.ny, g.nz])
    nbx, nby, _ = g.nb
    for c in range(n):
        lo, hi = valid_range[c]                                                                                # :137-138
        d = rng[c]
        ok = _valid(d, lo, hi)                                                                                 # :140 (fp32 values, compared exactly)
        ray = pixel_rays(H, W, *elev_range[c])                                                                 # :144-146
        r_start = np.maximum(d - g.trunc, lo)                                                                  # :148
        for k in range(g.num_samples):
            r = r_start + k * g.step                                                                           # :149
            margin = r - (d + g.trunc + g.step)
            live = ok & (margin <= 1e-6)                                                                       # :150
            firm = ok & (margin < -1e-6)
            p = pos[c] + R.quat_rotate(quat[c], ray * r[..., None])                                            # :154-165
            vf = (p - np.asarray(g.origin)) / g.vs + 0.5 * dims                                                # :166
            blocks = []
            for dx in (-R.FACE_TOL, R.FACE_TOL):
                for dy in (-R.FACE_TOL, R.FACE_TOL):
                    for dz in (-R.FACE_TOL, R.FACE_TOL):
                        v = np.floor(vf + np.array([dx, dy, dz])).astype(np.int64)                             # :168-170
                        inside = ((v >= 0) & (v < dims)).all(-1) & live                                        # :172
                        b = ((v[..., 2] // g.bs) * nby + v[..., 1] // g.bs) * nbx + v[..., 0] // g.bs           # :176-180
                        blocks.append(np.where(inside, b, -1))
            blocks = np.stack(blocks, 0)
            for b in blocks:
                possible[b[b >= 0]] = True
            same = (blocks == blocks[0]).all(0) & (blocks[0] >= 0) & firm
            sure[blocks[0][same]] = True
    return sure, possible


# ---------------------------------------------------------------------------------------------------- stage 2: voxels
def voxel_uv(v, H: int, W: int, min_elev: float, max_elev: float):
    """(u, v, elevation, in_band) of positions [..., 3] in the sensor frame  (lidar_integrate_voxels_kernel :421-437)"""
    el = np.arctan2(v[..., 2], np.hypot(v[..., 0], v[..., 1]))                                                 # :421-422
    if H == 1:
        vv, band = np.zeros_like(el), np.ones(el.shape, bool)                                                  # :423-424
    else:
        band = (el >= min_elev) & (el <= max_elev)                                                             # :426
        vv = (max_elev - el) * ((H - 1) / (max_elev - min_elev))                                               # :428-430
    u = (np.arctan2(v[..., 1], v[..., 0]) + PI) * (W / TWO_PI)                                                 # :432-433
    u = np.where(u >= W, u - W, u)                                                                             # :434-435
    u = np.where(u < 0, u + W, u)                                                                              # :436-437
    return u, vv, el, band


def sensor_range(rng, v, u, vv, H, W, lo, hi, min_elev, max_elev, linear_max_diff, nearest_max_dist):
    """_interpolate_lidar_range / _nearest_lidar_range (:244-367) for one sensor over voxels at (u, vv), positions v in its frame:
    dict(surface, ok, ambiguous, and the paths taken: bilinear, guard_then_nearest, corner_then_nearest, nearest_rejected, seam)"""
    rng = np.asarray(rng, np.float64)
    fu0, fv0 = np.floor(u), np.floor(vv)
    u0, v0 = fu0.astype(np.int64), fv0.astype(np.int64)
    try_bi = (H > 1) & (v0 >= 0) & (v0 < H - 1)                                                                # :295, :309-311
    u0 = np.where(u0 < 0, u0 + W, u0)                                                                          # :324-327
    u0 = np.where(u0 >= W, u0 - W, u0)
    u1 = np.where(u0 + 1 >= W, 0, u0 + 1)                                                                      # :328-330
    v0c = np.clip(v0, 0, max(H - 2, 0))
    v1c = np.minimum(v0c + 1, H - 1)                                                                           # :331
    d00, d01, d10, d11 = rng[v0c, u0], rng[v0c, u1], rng[v1c, u0], rng[v1c, u1]                                # :333-336
    corners = _valid(d00, lo, hi) & _valid(d01, lo, hi) & _valid(d10, lo, hi) & _valid(d11, lo, hi)            # :337-342
    fu, fv = u - fu0, vv - fv0                                                                                 # :344-345
    top, bottom = d00 * (1.0 - fu) + d01 * fu, d10 * (1.0 - fu) + d11 * fu                                     # :346-347
    interp = top * (1.0 - fv) + bottom * fv                                                                    # :348
    max_diff = np.max(np.abs(np.stack([d00, d01, d10, d11]) - interp), 0)                                      # :349-352
    bilinear = try_bi & corners & (max_diff <= linear_max_diff)                                                # :353
    amb = try_bi & corners & (np.abs(max_diff - linear_max_diff) < GUARD_TOL)
    # the nearest pixel (:257-279)
    un = np.floor(u + 0.5).astype(np.int64)                                                                    # :257
    wrapped = un >= W
    un = np.where(un >= W, un - W, un)                                                                         # :258-261
    un = np.where(un < 0, un + W, un)
    vn = np.floor(vv + 0.5).astype(np.int64) if H > 1 else np.zeros_like(un)                                   # :262-264
    in_image = (vn >= 0) & (vn < H)                                                                            # :265
    dn = rng[np.clip(vn, 0, H - 1), un]                                                                        # :268
    dn_ok = in_image & _valid(dn, lo, hi)                                                                      # :269
    ray = pixel_rays(H, W, min_elev, max_elev)[np.clip(vn, 0, H - 1), un]                                      # :272
    off = v - ray * np.sum(v * ray, -1, keepdims=True)                                                         # :273-275
    dist = np.sqrt(np.sum(off * off, -1))                                                                      # :276
    near_ok = dn_ok & (dist <= nearest_max_dist)                                                               # :277
    amb |= ~bilinear & dn_ok & (np.abs(dist - nearest_max_dist) < GUARD_TOL)
    ok = bilinear | near_ok
    seam = (bilinear & (u0 == W - 1)) | (~bilinear & near_ok & wrapped)  # a column of the pair, or the nearest column, came round the seam
    return dict(surface=np.where(bilinear, interp, dn), ok=ok, ambiguous=amb, bilinear=bilinear,
                guard_then_nearest=try_bi & corners & ~bilinear & near_ok, corner_then_nearest=try_bi & ~corners & near_ok,
                nearest_rejected=~bilinear & dn_ok & ~near_ok, seam=seam)


def integrate(g: "R.Grid", sw, w, visible, rng, pos, quat, valid_range, elev_range, linear_max_diff, nearest_max_dist, paths=None):
    """one frame of lidars into the fp16 pair ``sw``, ``w`` [n_blocks, bs^3] over the blocks of ``visible``.  Returns (sw, w) as
    float16, updated bool, ambiguous bool  (lidar_integrate_voxels_kernel :369-467).  ``paths``: a dict that receives, per path of
    the kernel, the voxels of ``visible`` blocks that took it for some sensor."""
    rng, pos, quat, valid_range, elev_range = (np.asarray(a, np.float64) for a in (rng, pos, quat, valid_range, elev_range))
    n, H, W = rng.shape
    centre = g.voxel_centres()                                                                                 # :391-394
    tot_sw, tot_w = np.zeros(centre.shape[:2]), np.zeros(centre.shape[:2])
    amb = np.zeros(centre.shape[:2], bool)
    vis = np.asarray(visible, bool)[:, None]
    for c in range(n):
        conj = quat[c] * np.array([1.0, -1.0, -1.0, -1.0])
        v = R.quat_rotate(conj, centre - pos[c])                                                               # :411
        rho = np.sqrt(np.sum(v * v, -1))                                                                       # :412
        lo, hi = valid_range[c]
        in_range = _valid(rho, lo, hi)                                                                         # :416
        near = (rho >= lo - BOUND_TOL) & (rho <= hi + BOUND_TOL)
        a = near & ((np.abs(rho - lo) < BOUND_TOL) | (np.abs(rho - hi) < BOUND_TOL))
        min_elev, max_elev = elev_range[c]
        u, vv, el, band = voxel_uv(v, H, W, min_elev, max_elev)
        if H > 1:
            a |= near & ((np.abs(el - min_elev) < BOUND_TOL) | (np.abs(el - max_elev) < BOUND_TOL))
            near &= (el >= min_elev - BOUND_TOL) & (el <= max_elev + BOUND_TOL)
            a |= near & (np.abs(2.0 * vv - np.rint(2.0 * vv)) < 2.0 * UV_TOL)
        a |= near & (np.abs(2.0 * u - np.rint(2.0 * u)) < 2.0 * UV_TOL)
        live = in_range & band
        s = sensor_range(rng[c], v, np.where(live, u, 0.0), np.where(live, vv, 0.0), H, W, lo, hi, min_elev, max_elev, linear_max_diff,
                         nearest_max_dist)
        a |= live & s["ambiguous"]
        got = live & s["ok"]                                                                                   # :452
        sdf = s["surface"] - rho                                                                               # :456
        a |= got & (np.abs(sdf + g.trunc) < SDF_TOL)
        keep = got & (sdf >= -g.trunc)                                                                         # :457
        tot_sw += np.where(keep, np.minimum(sdf, g.trunc), 0.0)                                                # :458-460, weight 1
        tot_w += np.where(keep, 1.0, 0.0)                                                                      # :461
        amb |= a
        if paths is not None:
            for name in ("guard_then_nearest", "corner_then_nearest"):
                paths[name] = paths.get(name, False) | (vis & keep & s[name])
            paths["bilinear"] = paths.get("bilinear", False) | (vis & keep & s["bilinear"])
            paths["nearest_rejected"] = paths.get("nearest_rejected", False) | (vis & live & s["nearest_rejected"])
            paths["seam"] = paths.get("seam", False) | (vis & keep & s["seam"])
            paths["clamped"] = paths.get("clamped", False) | (vis & keep & (sdf > g.trunc))
            paths["dropped"] = paths.get("dropped", False) | (vis & got & ~keep)
    upd = (tot_w > 0.0) & vis                                                                                  # :463
    sw64, w64 = np.asarray(sw, np.float16).astype(np.float64), np.asarray(w, np.float16).astype(np.float64)
    new_sw = np.where(upd, sw64 + tot_sw, sw64).astype(np.float16)                                             # :464-467
    new_w = np.where(upd, w64 + tot_w, w64).astype(np.float16)
    return new_sw, new_w, upd, amb


# ---------------------------------------------------------------------------------------------------- the decay's lidar frustum
def lidar_flags(centres, bs: int, vs: float, pos, quat, valid_range, elev_range, H: int):
    """one lidar: (inside bool, either bool) per block centre  (mark_lidar_blocks_in_frustum_kernel, builder_decay.py:264-313)"""
    pos, quat, valid_range, elev_range = (np.asarray(a, np.float64) for a in (pos, quat, valid_range, elev_range))
    r = SPHERE_FACTOR * (bs * vs)                                                                              # :264-265
    v = R.quat_rotate(quat * np.array([1.0, -1.0, -1.0, -1.0]), np.asarray(centres, np.float64) - pos)         # :278
    rho = np.sqrt(np.sum(v * v, -1))                                                                           # :280-284
    lo, hi = valid_range
    out_range = (rho + r < lo) | (rho - r > hi)                                                                # :287-290
    amb = (np.abs(rho + r - lo) < BOUND_TOL) | (np.abs(rho - r - hi) < BOUND_TOL)
    el = np.arctan2(v[..., 2], np.hypot(v[..., 0], v[..., 1]))                                                 # :292-293
    ratio = np.clip(r / np.maximum(rho, 1e-300), 0.0, 1.0)                                                     # :297-298
    ang = np.where(rho > r, np.arcsin(ratio), PI)                                                              # :295-299
    amb |= ~out_range & ((np.abs(rho - r) < BOUND_TOL) | ((rho > r) & (ratio > 0.999)))  # asin is steep at 1: fp32 may be 1e-5 off there
    min_elev, max_elev = elev_range
    if H == 1:
        fixed = (min_elev + max_elev) * 0.5                                                                    # :303-304
        inside = ~out_range & (np.abs(el - fixed) <= ang)                                                      # :305
        amb |= ~out_range & (np.abs(np.abs(el - fixed) - ang) < ANGLE_TOL)
    else:
        inside = ~out_range & ~((el + ang < min_elev) | (el - ang > max_elev))                                 # :309-313
        amb |= ~out_range & ((np.abs(el + ang - min_elev) < ANGLE_TOL) | (np.abs(el - ang - max_elev) < ANGLE_TOL))
    return inside, amb


def frustum_flags(g: "R.Grid", cameras=None, lidars=None):
    """the union over cameras and lidars (wp_decay.py:194-284): (sure_in, sure_out) bool [n_blocks]; a block in neither is *either*.
    ``cameras``: (K [n, 3, 3], pos, quat, H, W, depth_min, depth_max) or None; ``lidars``: (pos [n, 3], quat [n, 4], valid_range
    [n, 2], elev_range [n, 2], H) or None"""
    import mapper_decay_ref as DR

    centres = DR.block_centres(g)
    sure_in, sure_out = np.zeros(g.n_blocks, bool), np.ones(g.n_blocks, bool)
    if cameras is not None:
        K, pos, quat, H, W, dmin, dmax = cameras
        for c in range(len(K)):
            inside, amb = DR.camera_flags(centres, g.bs, g.vs, K[c], pos[c], quat[c], H, W, f32(dmin), f32(dmax))
            sure_in |= inside & ~amb
            sure_out &= ~inside & ~amb
    if lidars is not None:
        pos, quat, valid_range, elev_range, H = lidars
        for c in range(len(pos)):
            inside, amb = lidar_flags(centres, g.bs, g.vs, pos[c], quat[c], valid_range[c], elev_range[c], H)
            sure_in |= inside & ~amb
            sure_out &= ~inside & ~amb
    return sure_in, sure_out


# ---------------------------------------------------------------------------------------------------- the test scene
def render_range(pos, quat, H: int, W: int, min_elev: float, max_elev: float, radius: float = R.SPHERE_RADIUS,
                 ground_z: float = R.GROUND_Z) -> np.ndarray:
    """Euclidean range (float32, metres, 0 = nothing) along every pixel's ray of a sphere at the origin over the plane z = ground_z"""
    pos, quat = np.asarray(pos, np.float64), np.asarray(quat, np.float64)
    ray = R.quat_rotate(quat, pixel_rays(H, W, float(min_elev), float(max_elev)))  # unit: t is the range
    b, c = 2.0 * (ray * pos).sum(-1), (pos * pos).sum() - radius * radius
    disc = b * b - 4 * c
    t_s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / 2, np.inf)
    t_s = np.where(t_s > 0, t_s, np.inf)
    down = ray[..., 2] < -1e-9
    t_p = np.where(down, (ground_z - pos[2]) / np.where(down, ray[..., 2], -1.0), np.inf)
    t_p = np.where(t_p > 0, t_p, np.inf)
    t = np.minimum(t_s, t_p)
    return np.where(np.isfinite(t), t, 0.0).astype(np.float32)
