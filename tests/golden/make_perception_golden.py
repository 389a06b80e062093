"""Golden vectors for curobo_amd.perception, produced by the REFERENCE's own code on the CPU:

    PYTHONPATH=/root/reference python tests/golden/make_perception_golden.py

filter     curobo/_src/perception/filter_depth.py: ``FilterDepth`` itself (constructor, ``_setup_kernel_params``, ``__call__``
           -> ``_apply_fused`` / ``_apply_separable``) on CPU tensors, its three unmodified Warp kernels
           (perception/mapper/kernel/wp_filter_depth.py) executed thread by thread through tests/golden/warp_emulator (see
           make_scene_warp_golden.py).  Cases: flying-pixel rejection on / off x bilateral off / 3 / 5 (one launch) / 7 / 9
           (three passes), B = 1 and 2, 40 x 56 images with depth steps of 1.5 cm .. 1 m (flying pixels on one or both
           sides of an edge), a ramp, millimetre noise, NaN / +-inf / 0 / below-minimum / above-maximum pixels alone and in
           blocks, and features that touch the image border.
segmenter  curobo/_src/geom/cv.py ``get_projection_rays`` / ``project_depth_using_rays`` and
           perception/robot_segmenter.py ``_mask_spheres_image`` (recorded) / ``_mask_spheres_image_cdist`` (asserted here to
           agree with it outside the band below), in fp32 and in the reference's default bf16-ops arithmetic, sequenced as
           ``RobotSegmenter._mask_op`` does.  The camera transform is ``Pose.batch_transform_points``' Warp kernel
           (geom/transform.py ``compute_batch_transform_point``) through the emulator: it runs there.  ``torch.cdist`` refuses
           mixed dtypes, so in bf16-ops mode the cdist form gets the bf16-rounded spheres widened to fp32 (the same values).
           Depth images are rendered here: the Franka sphere model (this repository's packaged model through the C oracle's
           FK) at two joint configurations, a table plane and a box, ray-cast from two tilted camera poses, with a border
           of zero depth.  B = 1 and 2, one and two sphere sets / camera poses / intrinsics; one sphere is disabled the way
           this library disables spheres (radius -100) in the sets that are masked against.
pipeline   rendered depth with millimetre noise -> FilterDepth (5 x 5) -> mask (fp32), and the fixture condition of the
           end-to-end test checked on the reference's output.

Excluded sets (the ONLY pixels a test may skip), computed from the inputs and the reference's own values:
  filter   pixels where a decisive comparison is closer than 1e-6 m to its threshold: the pixel or one of its 4 clamped
           neighbours within 1e-6 of the minimum / maximum distance, or |largest neighbour difference - tolerance * depth|
           < 1e-6 (evaluated in float64 with the reference's neighbour rules).  Asserted <= 0.5 % of every case.
  mask     pixels whose recorded reference distance max_s(r_s - |p - c_s|) is within 1e-5 m of -distance_threshold.
           Asserted <= 0.1 % of every case.
Output: tests/golden/perception_golden.npz.

edges      a second file, tests/golden/perception_edges_golden.npz (``edge_cases``), by the same code at the shapes where the HIP
           kernels change how they index.  Filter: widths 64, 65 and 130 x heights 15 .. 20 (a tile is 64 x 16), kernel sizes 1
           (accepted by the reference: radius 0) and 31 with a small and a large spatial sigma, minimum distance 0 with kernel
           sizes 7 and 9 (the 0 a rejected pixel carries is in range in the two 1-d passes: the reference returns non-zero
           depth at such pixels, printed below), a NaN and an out-of-range pixel on each side of x = 63 | 64.  Mask, through
           ``reference_mask`` as it stands: 1 pixel, 1023 pixels, 2049 spheres (enabled at 0, 2047, 2048: each asserted to mask
           pixels of its own), rays shared with pose and spheres per image and the reverse; no sphere at all, which the
           reference refuses (its max over an empty dimension raises: the message is recorded with the inputs).  Same caps.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "urdf_standin"))  # yourdfpy / lxml, which the segmenter module imports through Kinematics
sys.path.append(ROOT)
import make_scene_warp_golden as _emu  # noqa: E402,F401  (puts the emulator + module stubs in place)

import warp as wp  # noqa: E402

from curobo._src.geom.cv import get_projection_rays, project_depth_using_rays  # noqa: E402
from curobo._src.geom.transform import compute_batch_transform_point  # noqa: E402
from curobo._src.perception.filter_depth import FilterDepth  # noqa: E402
from curobo._src.perception.robot_segmenter import _mask_spheres_image, _mask_spheres_image_cdist  # noqa: E402

FILTER_BAND, MASK_BAND = 1e-6, 1e-5
THRESHOLD = 0.05


# ----------------------------------------------------------------------------------------------------- filter
def filter_image(rng, H, W, variant):
    v, u = np.mgrid[0:H, 0:W]
    d = 2.0 + 0.004 * u + 0.002 * v                       # a slanted wall: 4 mm per pixel
    d[6:20, 8:24] = 1.0                                   # a near box: 1 m step, flying pixels on both sides
    d[24:34, 6:18] = d[24:34, 6:18] - 0.015               # 1.5 cm step: below the tolerance at 2 m (2 % -> 4 cm)
    d[22:36, 30:44] = 1.2 + 0.012 * (u[22:36, 30:44] - 30)  # a steep ramp in front of the wall
    d[0:5, 40:56] = 0.8                                   # a feature on the top / right border
    d[30:40, 0:4] = 1.5                                   # ... and on the bottom / left border
    d[H - 1, 20:30] = 0.6
    if variant:
        d = d[::-1, ::-1].copy() * 1.1
        d[10:14, 10:40] = 0.9 + 0.03                      # 3 cm step against 0.9 m: flagged on the near side only
    d = d + rng.normal(0.0, 0.001, d.shape)               # millimetre noise
    for (i, j, val) in [(3, 3, np.nan), (12, 30, np.inf), (15, 12, -np.inf), (20, 40, 0.0), (28, 50, 0.05), (35, 25, 12.0),
                        (0, 0, np.nan), (H - 1, W - 1, 0.0), (8, 9, np.nan), (26, 35, 0.0)]:
        d[i, j] = val
    d[16:19, 44:48] = 0.0                                 # a hole
    d[36:38, 46:52] = 11.0                                # beyond the maximum
    return d.astype(np.float32)


def filter_band(depth, dmin, dmax, enable_flying, tol):
    """pixels whose range / flying decision lies within FILTER_BAND of its threshold (float64, the reference's neighbour rules)"""
    d = depth.astype(np.float64)
    near_limit = (np.abs(d - dmin) < FILTER_BAND) | (np.abs(d - dmax) < FILTER_BAND)
    pad = np.pad(d, ((0, 0), (1, 1), (1, 1)), mode="edge")
    pad_lim = np.pad(near_limit, ((0, 0), (1, 1), (1, 1)), mode="edge")
    nb = [pad[:, 1:-1, :-2], pad[:, 1:-1, 2:], pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]]
    nb_lim = [pad_lim[:, 1:-1, :-2], pad_lim[:, 1:-1, 2:], pad_lim[:, :-2, 1:-1], pad_lim[:, 2:, 1:-1]]
    band = near_limit.copy()
    if enable_flying:
        for x in nb_lim:
            band |= x
        with np.errstate(invalid="ignore"):
            diffs = [np.abs(d - np.where((x < dmin) | (x > dmax), d, x)) for x in nb]
            m = np.fmax(np.fmax(diffs[0], diffs[1]), np.fmax(diffs[2], diffs[3]))
            band |= np.abs(m - np.float64(np.float32(tol)) * d) < FILTER_BAND
    return band


def filter_cases(out):
    rng = np.random.default_rng(2031)
    H, W = 40, 56
    names, params = [], []
    k = 0
    for flying in (0.5, None, 0.8):
        for ksize in (None, 3, 5, 7, 9):
            if flying == 0.8 and ksize not in (5, 9):
                continue
            B = 2 if k % 2 else 1
            depth = np.stack([filter_image(rng, H, W, b) for b in range(B)])
            kw = dict(depth_minimum_distance=0.1, depth_maximum_distance=10.0, flying_pixel_threshold=flying,
                      bilateral_kernel_size=ksize, bilateral_sigma_spatial=2.0 if k % 3 else 10.0,
                      bilateral_sigma_depth=0.05 if k % 3 else 0.1)
            fd = FilterDepth(image_shape=(H, W), device="cpu", num_batch=B, **kw)
            assert fd.device.type == "cpu"
            filtered, valid = fd(torch.as_tensor(depth))
            name = f"filter{k:02d}"
            names.append(name)
            params.append([kw["depth_minimum_distance"], kw["depth_maximum_distance"], -1.0 if flying is None else flying,
                           0 if ksize is None else ksize, kw["bilateral_sigma_spatial"], kw["bilateral_sigma_depth"],
                           fd._enable_flying, fd._flying_tolerance, fd._enable_bilateral, fd._bilateral_radius,
                           fd._sigma_spatial_sq2, fd._sigma_depth_sq2, float(fd._use_separable)])
            band = filter_band(depth, 0.1, 10.0, fd._enable_flying, fd._flying_tolerance)
            assert band.mean() <= 0.005, (name, band.mean())
            out[f"{name}/depth"], out[f"{name}/filtered"] = depth, filtered.numpy().copy()
            out[f"{name}/valid"], out[f"{name}/excluded"] = valid.numpy().astype(np.uint8), band
            v = valid.numpy()
            print(name, "B", B, "flying", flying, "kernel", ksize, "valid", int(v.sum()), "of", v.size, "band", int(band.sum()),
                  "changed", int((np.abs(filtered.numpy() - depth)[v] > 1e-6).sum()))
            k += 1
    out["filter_case_names"] = np.array(names)
    # min, max, flying_pixel_threshold (-1: None), kernel size (0: None), sigma_spatial, sigma_depth, then the reference's derived
    # constants: enable_flying, flying_tolerance, enable_bilateral, radius, 2 sigma_s^2, 2 sigma_d^2, separable
    out["filter_case_params"] = np.array(params, np.float64)


# ----------------------------------------------------------------------------------------------------- rendering
def look_at(eye, target):
    """world_from_camera rotation (camera x right, y down, z forward) and the wxyz quaternion of it"""
    z = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    w = 0.5 * np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12))
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return R, q / np.linalg.norm(q)


BOX = (np.array([0.35, -0.55, 0.0]), np.array([0.6, -0.3, 0.25]))


def render(H, W, K, eye, R, spheres, border=4):
    """depth (z of the camera frame) of the first hit of every pixel ray: robot spheres / table plane z = 0 / the box;
    labels 1 robot, 2 table, 3 box, 0 nothing (and the zero-depth border)"""
    v, u = np.mgrid[0:H, 0:W]
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u, np.float64)], -1).reshape(-1, 3)
    dvec = ray @ R.T
    o = np.asarray(eye, np.float64)
    t_best = np.full(ray.shape[0], np.inf)
    label = np.zeros(ray.shape[0], np.int32)
    live = spheres[:, 3] > 0
    c, r = spheres[live, :3].astype(np.float64), spheres[live, 3].astype(np.float64)
    oc = o[None, :] - c
    a = (dvec * dvec).sum(-1)[:, None]
    b = 2.0 * dvec @ oc.T
    cc = (oc * oc).sum(-1)[None, :] - r[None, :] ** 2
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t = np.where(t > 0, t, np.inf).min(1)
    label[t < t_best] = 1
    t_best = np.minimum(t_best, t)
    with np.errstate(divide="ignore"):
        tp = np.where(dvec[:, 2] < 0, -o[2] / dvec[:, 2], np.inf)
    label[tp < t_best] = 2
    t_best = np.minimum(t_best, tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (BOX[0] - o) / dvec, (BOX[1] - o) / dvec
    tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    tb = np.where((tn <= tf) & (tn > 0), tn, np.inf)
    label[tb < t_best] = 3
    t_best = np.minimum(t_best, tb)
    depth = np.where(np.isfinite(t_best), t_best, 0.0).reshape(H, W)
    label = label.reshape(H, W)
    label[depth == 0] = 0
    for arr in (depth, label) if border else ():
        arr[:border] = 0
        arr[-border:] = 0
        arr[:, :border] = 0
        arr[:, -border:] = 0
    return depth.astype(np.float32), label


def franka_spheres(qs):
    from curobo_amd.robot import load_packaged_robot
    from oracle import build_oracle, load_oracle

    build_oracle()
    model = load_packaged_robot("franka")
    fk = load_oracle().kinematics_forward(np.asarray(qs, np.float32), model.as_dict(), horizon=1)
    return fk["robot_spheres"].astype(np.float32), [str(n) for n in model.joint_names]


# ----------------------------------------------------------------------------------------------------- segmenter
def reference_mask(depth, intrinsics, depth_to_meter, cam_p, cam_q, spheres, ops_dtype):
    """RobotSegmenter._mask_op (robot_segmenter.py:215-280) from the spheres on, on CPU tensors"""
    B, H, W = depth.shape
    image = torch.as_tensor(depth)
    rays32 = get_projection_rays(H, W, torch.as_tensor(intrinsics), depth_to_meter)
    rays = rays32.to(dtype=ops_dtype)                                   # update_camera_projection
    points = project_depth_using_rays(image.to(dtype=ops_dtype), rays)  # get_pointcloud_from_depth
    points32 = points.to(dtype=torch.float32).contiguous()
    n = H * W
    pos = np.ascontiguousarray(np.broadcast_to(cam_p, (B, 3)), np.float32)   # one pose per image, as Pose.batch_transform_points needs
    quat = np.ascontiguousarray(np.broadcast_to(cam_q, (B, 4)), np.float32)
    moved = np.zeros((B * n, 3), np.float32)
    wp.launch(kernel=compute_batch_transform_point, dim=B * n,
              inputs=[wp.array(pos, dtype=wp.vec3), wp.array(quat, dtype=wp.vec4), wp.array(points32.numpy().reshape(-1, 3), dtype=wp.vec3), n, B],
              outputs=[wp.array(moved, dtype=wp.vec3)])
    in_robot = torch.as_tensor(moved.reshape(B, n, 3))
    sph = torch.as_tensor(spheres).to(dtype=ops_dtype).view(spheres.shape[0], -1, 4)
    mask, filtered = _mask_spheres_image(image, sph, in_robot, THRESHOLD)
    mask_c, filtered_c = _mask_spheres_image_cdist(image, sph.to(torch.float32), in_robot, THRESHOLD)
    # the reference's per-pixel signed distance (the expression inside _mask_spheres_image)
    s = sph.unsqueeze(-3)
    dist = (-1 * (torch.linalg.norm(in_robot.unsqueeze(-2) - s[..., :3], dim=-1) - s[..., 3])).max(dim=-1)[0].view(B, H, W)
    band = (dist + THRESHOLD).abs() < MASK_BAND
    assert bool((mask == mask_c)[~band].all()) and bool((filtered == filtered_c)[~band].all()), "the two reference forms disagree outside the band"
    assert float(band.float().mean()) <= 0.001, float(band.float().mean())
    return dict(rays=rays32.numpy(), points=project_depth_using_rays(image, rays32).numpy(), mask=mask.numpy().astype(np.uint8),
                filtered=filtered.numpy(), distance=dist.numpy().astype(np.float32), excluded=band.numpy())


def segmenter_cases(out):
    H, W = 72, 96
    q = np.array([[0.0, -1.3, 0.0, -2.5, 0.0, 1.5, 0.8], [0.9, -0.4, -0.5, -1.6, 0.6, 1.9, -0.3]], np.float32)
    spheres, joint_names = franka_spheres(q)              # [2, 65, 4]
    K = np.array([[[84.0, 0, 47.5], [0, 84.0, 35.5], [0, 0, 1]], [[72.0, 0, 45.0], [0, 74.0, 38.0], [0, 0, 1]]], np.float32)
    eyes = [np.array([0.95, 0.4, 1.3]), np.array([0.75, -0.85, 1.25])]  # steep views: the table's depth changes < 2 % per pixel
    Rq = [look_at(e, [0.15, 0.0, 0.3]) for e in eyes]
    cam_p = np.stack(eyes).astype(np.float32)
    cam_q = np.stack([r[1] for r in Rq]).astype(np.float32)
    # one slot is disabled the way this library disables spheres (radius -100, attachment_manager.py: an unused
    # attachment slot keeps a position): it lies on the table in view of both cameras, where an enabled sphere would mask
    disabled = 40
    spheres[:, disabled] = [0.45, -0.1, 0.02, 0.06]
    masked_against = spheres.copy()
    masked_against[:, disabled, 3] = -100.0
    rendered = masked_against                             # the disabled sphere is not in the scene either
    # image c: camera c looking at configuration c
    imgs = [render(H, W, K[c].astype(np.float64), eyes[c], Rq[c][0], rendered[c]) for c in (0, 1)]
    depth = np.stack([i[0] for i in imgs])
    label = np.stack([i[1] for i in imgs])
    out.update({"seg/q": q, "seg/joint_names": np.array(joint_names), "seg/spheres": masked_against, "seg/intrinsics": K,
                "seg/cam_position": cam_p, "seg/cam_quaternion": cam_q, "seg/depth": depth, "seg/label": label,
                "seg/disabled_sphere": np.int32(disabled), "seg/distance_threshold": np.float32(THRESHOLD),
                "seg/depth_to_meter": np.float32(1.0), "seg/unmasked_radius": spheres[:, disabled, 3]})
    # name: images, intrinsics, poses, sphere sets (index lists into the arrays above)
    cases = {"b1": ([0], [0], [0], [0]), "b2_shared": ([0, 1], [0], [0], [0]), "b2_each": ([0, 1], [0, 1], [0, 1], [0, 1]),
             "b1_second": ([1], [1], [1], [1])}
    names = []
    for name, (im, ki, pi, si) in cases.items():
        for mode, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            r = reference_mask(depth[im], K[ki], 1.0, cam_p[pi], cam_q[pi], masked_against[si], dt)
            key = f"seg/{name}/{mode}"
            for k2 in ("mask", "filtered", "distance", "excluded"):
                out[f"{key}/{k2}"] = r[k2]
            if mode == "fp32" and name in ("b1", "b2_each"):  # get_projection_rays / project_depth_using_rays, fp32 as CameraObservation uses them
                out[f"seg/{name}/rays"] = r["rays"]
                if name == "b1":
                    out[f"seg/{name}/points"] = r["points"]
            lab = label[im]
            robot, scene = lab == 1, lab >= 2
            print(key, "masked", int(r["mask"].sum()), "robot px", int(robot.sum()), "robot px masked", int(r["mask"][robot].sum()),
                  "scene px", int(scene.sum()), "scene px masked", int(r["mask"][scene].sum()), "band", int(r["excluded"].sum()))
            if name in ("b1", "b2_each", "b1_second") and mode == "fp32":
                assert r["mask"][robot].all(), "a rendered robot pixel is not masked by the reference"
                assert not r["mask"][depth[im] == 0].any()
        out[f"seg/{name}/index"] = np.array([im + [-1] * (2 - len(im)), ki + [-1] * (2 - len(ki)), pi + [-1] * (2 - len(pi)), si + [-1] * (2 - len(si))], np.int32)
        names.append(name)
    out["seg_case_names"] = np.array(names)
    # the disabled sphere masks nothing: with its true radius instead it WOULD mask pixels of image 0 (so the case means something)
    r_on = reference_mask(depth[[0]], K[[0]], 1.0, cam_p[[0]], cam_q[[0]], spheres[[0]], torch.float32)
    added = int((r_on["mask"] != out["seg/b1/fp32/mask"]).sum())
    print("disabled sphere: pixels it would add when enabled", added)
    assert added > 10
    return depth, label, K, cam_p, cam_q, masked_against, eyes, Rq


def pipeline_case(out, depth, label, K, cam_p, cam_q, spheres):
    """rendered depth + noise -> FilterDepth -> mask (fp32) on the reference; the end-to-end test's fixture condition"""
    rng = np.random.default_rng(5)
    noisy = np.where(depth[[0]] > 0, depth[[0]] + rng.normal(0, 0.001, depth[[0]].shape), 0.0).astype(np.float32)
    kw = dict(depth_minimum_distance=0.1, depth_maximum_distance=10.0, flying_pixel_threshold=0.25, bilateral_kernel_size=5,
              bilateral_sigma_spatial=2.0, bilateral_sigma_depth=0.05)
    fd = FilterDepth(image_shape=depth.shape[1:], device="cpu", num_batch=1, **kw)
    filtered, valid = fd(torch.as_tensor(noisy))
    r = reference_mask(filtered.numpy().copy(), K[[0]], 1.0, cam_p[[0]], cam_q[[0]], spheres[[0]], torch.float32)
    survivors = (r["filtered"] > 0)
    # scene pixels (table / box) farther than the threshold from the robot, by the rendered (noise-free) geometry
    clean = reference_mask(depth[[0]], K[[0]], 1.0, cam_p[[0]], cam_q[[0]], spheres[[0]], torch.float32)
    far_scene = (label[[0]] >= 2) & (clean["distance"] < -THRESHOLD - 0.005)
    kept = survivors[far_scene].mean()
    assert r["distance"][survivors].max() <= -THRESHOLD + MASK_BAND
    assert kept >= 0.95, kept
    print("pipeline: survivors", int(survivors.sum()), "far scene px", int(far_scene.sum()), "kept", float(kept))
    out.update({"pipe/depth": noisy, "pipe/far_scene": far_scene, "pipe/filter_params": np.array(list(kw.values()), np.float64),
                "pipe/filtered": filtered.numpy().copy(), "pipe/valid": valid.numpy().astype(np.uint8),
                "pipe/survivors": survivors, "pipe/kept_fraction": np.float64(kept)})


# ----------------------------------------------------------------------------------------------------- edge cases
def edge_filter_image(rng, H, W, dmin, variant):
    """any H >= 15, W >= 64: the features of filter_image moved onto the x = 63 / 64 (and 127 / 128) tile seams of the HIP
    kernel and the y = 15 / 16 one, a NaN and an out-of-range pixel on each side of every seam in view; with dmin = 0 a near
    surface (0.3 m: within a few sigma_depth of the zeros that rejected pixels carry) with rejected pixels inside"""
    v, u = np.mgrid[0:H, 0:W]
    d = 2.0 + 0.004 * u + 0.002 * v
    d[3:11, 8:24] = 1.0                                   # 1 m step
    d[2:H - 2, 58:70] -= 0.015                            # 1.5 cm step, across the seam
    d[6:H, 61:64] = 1.3                                   # a near strip that ends ON the seam: flying pixels at x = 63 | 64
    d[0:4, W - 9:W] = 0.8                                 # top / right border
    d[H - 1, 20:30] = 0.6
    if W > 128:
        d[4:12, 120:128] = 1.2 + 0.012 * (u[4:12, 120:128] - 120)  # a ramp that ends on the second seam
    if variant:
        d = d * 1.1
        d[12:H, 30:52] = 0.9 + 0.03
    if dmin == 0.0:
        d[4:14, 30:50] = 0.3 + 0.001 * (u[4:14, 30:50] - 30) + 0.0005 * (v[4:14, 30:50] - 4)
    d = d + rng.normal(0.0, 0.001, d.shape)
    below, above = dmin - 0.05, 12.0
    for s in [63] + ([127] if W > 128 else []):           # (row, column): left of the seam, right of it
        for (i, j, val) in [(1, s, np.nan), (1, s + 1, below), (8, s, above), (8, s + 1, np.nan), (12, s, np.inf), (13, s + 1, -np.inf),
                            (H - 1, s, below), (H - 2, s + 1, 0.0 if dmin > 0 else below)]:
            if j < W:
                d[i, j] = val
    for (i, j, val) in [(0, 0, np.nan), (H - 1, W - 1, below), (5, 12, np.nan), (0, W - 1, above), (9, 40, np.nan), (7, 36, below),
                        (11, 45, np.inf)]:
        d[i, j] = val
    d[5:7, 33:35] = 0.0 if dmin > 0 else below            # a hole (an input of exactly 0 = dmin would lie in the excluded band)
    if H > 16:
        d[15:17, 10:14] = 11.0                            # beyond the maximum, across y = 15 | 16
    return d.astype(np.float32)


# name: H, W, B, min distance, flying_pixel_threshold, kernel size, sigma_spatial, sigma_depth
EDGE_FILTER_CASES = [
    ("w64_k5", 16, 64, 1, 0.1, 0.5, 5, 2.0, 0.05),
    ("w65_k7", 17, 65, 2, 0.1, 0.5, 7, 2.0, 0.05),
    ("w65_k3", 15, 65, 1, 0.1, 0.8, 3, 10.0, 0.1),
    ("w130_k5", 18, 130, 1, 0.1, 0.5, 5, 10.0, 0.1),
    ("w130_k9", 20, 130, 1, 0.1, None, 9, 2.0, 0.05),
    ("w64_k31_small_sigma", 19, 64, 1, 0.1, 0.5, 31, 2.0, 0.05),
    ("w130_k31_large_sigma", 17, 130, 1, 0.1, None, 31, 10.0, 0.1),
    ("w65_k1", 16, 65, 1, 0.1, 0.5, 1, 2.0, 0.05),
    ("w65_k7_min0", 18, 65, 2, 0.0, 0.5, 7, 2.0, 0.1),
    ("w130_k9_min0_noflying", 16, 130, 1, 0.0, None, 9, 10.0, 0.05),
]


def edge_filter_cases(out):
    rng = np.random.default_rng(2032)
    names, params = [], []
    for name, H, W, B, dmin, flying, ksize, ss, sd in EDGE_FILTER_CASES:
        depth = np.stack([edge_filter_image(rng, H, W, dmin, b) for b in range(B)])
        kw = dict(depth_minimum_distance=dmin, depth_maximum_distance=10.0, flying_pixel_threshold=flying, bilateral_kernel_size=ksize,
                  bilateral_sigma_spatial=ss, bilateral_sigma_depth=sd)
        fd = FilterDepth(image_shape=(H, W), device="cpu", num_batch=B, **kw)  # (kernel size 1 is accepted: radius 0, one launch)
        filtered, valid = fd(torch.as_tensor(depth))
        name = "filter_" + name
        names.append(name)
        params.append([dmin, 10.0, -1.0 if flying is None else flying, ksize, ss, sd, fd._enable_flying, fd._flying_tolerance,
                       fd._enable_bilateral, fd._bilateral_radius, fd._sigma_spatial_sq2, fd._sigma_depth_sq2, float(fd._use_separable)])
        band = filter_band(depth, dmin, 10.0, fd._enable_flying, fd._flying_tolerance)
        assert band.mean() <= 0.005, (name, band.mean())
        out[f"{name}/depth"], out[f"{name}/filtered"] = depth, filtered.numpy().copy()
        out[f"{name}/valid"], out[f"{name}/excluded"] = valid.numpy().astype(np.uint8), band
        v, f = valid.numpy(), filtered.numpy()
        print(name, (B, H, W), "flying", flying, "kernel", ksize, "valid", int(v.sum()), "of", v.size, "band", int(band.sum()),
              "changed", int((np.abs(f - depth)[v] > 1e-6).sum()), "rejected pixels the later passes left non-zero", int((f[~v] != 0).sum()),
              "largest", float(np.abs(f[~v]).max()))
    out["filter_case_names"] = np.array(names)
    out["filter_case_params"] = np.array(params, np.float64)  # columns as in perception_golden.npz


def edge_segmenter_cases(out, K, cam_p, cam_q, spheres, eyes, Rq):
    """small images through reference_mask as it stands: 1 pixel, 1023 pixels, no sphere, 2049 spheres (three enabled: the first,
    the last of the HIP kernel's first chunk of 2048 and the first of its second), and the two batched / shared combinations
    perception_golden.npz lacks"""
    def scaled(k, f):
        k = k.astype(np.float64).copy()
        k[:2] *= f
        return k.astype(np.float32)

    def shot(H, W, f, c, sph, border=2):
        return render(H, W, scaled(K[c], f).astype(np.float64), eyes[c], Rq[c][0], sph, border)[0]

    cases = {}
    # one pixel whose ray goes through the centre of a robot sphere of camera 0's view, once at the robot, once 2 m behind it
    c = Rq[0][0].T @ (spheres[0, 30, :3].astype(np.float64) - eyes[0])
    k1 = np.array([[50.0, 0, -50.0 * c[0] / c[2]], [0, 50.0, -50.0 * c[1] / c[2]], [0, 0, 1]], np.float32)
    hit = render(1, 1, k1.astype(np.float64), eyes[0], Rq[0][0], spheres[0], 0)[0]
    cases["px1"] = (np.stack([hit, hit + 2.0]).astype(np.float32), k1[None], cam_p[[0]], cam_q[[0]], spheres[[0]])
    cases["px1023"] = (shot(31, 33, 1.0 / 3.0, 0, spheres[0])[None], scaled(K[0], 1.0 / 3.0)[None], cam_p[[0]], cam_q[[0]], spheres[[0]])
    cases["s0"] = (shot(24, 32, 1.0 / 3.0, 0, spheres[0])[None], scaled(K[0], 1.0 / 3.0)[None], cam_p[[0]], cam_q[[0]],
                   np.zeros((1, 0, 4), np.float32))
    many = np.zeros((1, 2049, 4), np.float32)
    many[..., :3] = np.random.default_rng(7).uniform([-0.2, -0.5, 0.0], [0.7, 0.5, 0.6], (1, 2049, 3))  # where enabled ones WOULD mask
    many[..., 3] = -100.0
    alone = {0: [0.45, -0.1, 0.02, 0.1], 2047: [0.3, 0.3, 0.02, 0.1], 2048: [-0.1, -0.3, 0.02, 0.1]}
    for k, s in alone.items():
        many[0, k] = s
    cases["s2049"] = (shot(24, 32, 1.0 / 3.0, 0, many[0])[None], scaled(K[0], 1.0 / 3.0)[None], cam_p[[0]], cam_q[[0]], many)
    half = np.stack([scaled(K[0], 0.5), scaled(K[1], 0.5)])
    # rays shared, pose and spheres per image: image c is pose c looking at configuration c through camera 0's intrinsics
    d = np.stack([render(36, 48, half[0].astype(np.float64), eyes[c], Rq[c][0], spheres[c], 2)[0] for c in (0, 1)])
    cases["rays_shared"] = (d, half[[0]], cam_p, cam_q, spheres)
    # rays per image, pose and spheres shared: pose 0 and configuration 0 through both cameras' intrinsics
    d = np.stack([render(36, 48, half[c].astype(np.float64), eyes[0], Rq[0][0], spheres[0], 2)[0] for c in (0, 1)])
    cases["rays_each"] = (d, half, cam_p[[0]], cam_q[[0]], spheres[[0]])
    names = []
    for name, (depth, k, p, q, sph) in cases.items():
        key = f"seg_{name}"
        out.update({f"{key}/depth": depth, f"{key}/intrinsics": k, f"{key}/cam_position": p, f"{key}/cam_quaternion": q, f"{key}/spheres": sph})
        names.append(key)
        if sph.shape[1] == 0:  # the reference's max over the spheres refuses an empty set: recorded as that, with the inputs
            try:
                reference_mask(depth, k, 1.0, p, q, sph, torch.float32)
            except IndexError as ex:
                out[f"{key}/reference_raises"] = np.array(f"{type(ex).__name__}: {ex}")
                out[f"{key}/rays"] = get_projection_rays(depth.shape[1], depth.shape[2], torch.as_tensor(k), 1.0).numpy()
                print(key, "the reference raises", out[f"{key}/reference_raises"])
                continue
            raise AssertionError("the reference accepts an empty sphere set: record its output")
        for mode, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            r = reference_mask(depth, k, 1.0, p, q, sph, dt)
            for k2 in ("mask", "filtered", "distance", "excluded"):
                out[f"{key}/{mode}/{k2}"] = r[k2]
            out[f"{key}/rays"] = r["rays"]
            print(key, mode, depth.shape, "spheres", sph.shape, "masked", int(r["mask"].sum()), "of", int((depth > 0).sum()), "with depth, band",
                  int(r["excluded"].sum()))
            if name == "s2049":  # every enabled sphere masks pixels no other sphere does
                for k3 in alone:
                    less = sph.copy()
                    less[0, k3, 3] = -100.0
                    lost = int((reference_mask(depth, k, 1.0, p, q, less, dt)["mask"] != r["mask"]).sum())
                    print("   without sphere", k3, "the mask loses", lost, "pixels")
                    assert lost >= 3
    assert out["seg_px1/fp32/mask"].reshape(-1).tolist() == [1, 0]
    out["seg_case_names"] = np.array(names)
    out["seg/distance_threshold"] = np.float32(THRESHOLD)


def edge_cases(K, cam_p, cam_q, spheres, eyes, Rq):
    """tests/golden/perception_edges_golden.npz: the shapes at which the HIP kernels change how they index"""
    out = {}
    edge_filter_cases(out)
    edge_segmenter_cases(out, K, cam_p, cam_q, spheres, eyes, Rq)
    path = os.path.join(HERE, "perception_edges_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def main():
    out = {}
    filter_cases(out)
    depth, label, K, cam_p, cam_q, spheres, eyes, Rq = segmenter_cases(out)
    pipeline_case(out, depth, label, K, cam_p, cam_q, spheres)
    path = os.path.join(HERE, "perception_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    edge_cases(K, cam_p, cam_q, spheres, eyes, Rq)


if __name__ == "__main__":
    main()
