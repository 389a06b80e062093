"""Times the perception launches on the GPU against a torch-eager composition of the same formulas:

    python tools/perception_timing.py [--out profiles/perception_timing.jsonl] [--quick]

Per image size (480 x 640, 720 x 1280), batch (1, 4) and robot (Franka, Unitree G1 sphere counts): the mask launch, the filter
launch (5 x 5 in one launch, 9 x 9 in three), the graph-replayed ``RobotSegmenter.get_robot_mask`` end to end (FK + mask +
output clones), and what a user would write in torch today: depth x rays -> pose -> distance to every sphere -> max ->
threshold -> where (the pixels x spheres intermediate of the reference's formulation), and for the filter the same taps with
unfold-free shifted slices.  Device events around ``iters`` launches after a warm-up, median of ``repeats`` windows.
Every row carries the bytes the launch must move (depth in + depth out + mask out, plus rays for the mask) and the share of the
HBM peak that time corresponds to; for the mask also the sphere tests per pixel, since at hundreds of spheres the launch is
bound by instruction issue, not by bandwidth.  ``--kernels-only`` runs each HIP launch a few times and nothing else (for a
``rocprofv3 --kernel-trace --stats`` run of its own)."""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def timed(fn, iters, repeats=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / iters)
    return sorted(out)[len(out) // 2], min(out), max(out)


def eager_mask(depth, rays, pos, quat, spheres, thr):
    B, H, W = depth.shape
    pts = depth.view(B, -1, 1) * rays
    w, u = quat[:, None, :1], quat[:, None, 1:]
    t = 2.0 * torch.cross(u.expand_as(pts), pts, dim=-1)
    pts = pts + w * t + torch.cross(u.expand_as(pts), t, dim=-1) + pos[:, None, :]
    s = spheres.unsqueeze(-3)
    dist = -1 * (torch.linalg.norm(pts.unsqueeze(-2) - s[..., :3], dim=-1) - s[..., 3])
    dist = dist.max(dim=-1)[0].view(B, H, W)
    mask = torch.logical_and(depth > 0.0, dist > -thr)
    return mask, torch.where(mask, 0, depth)


def eager_filter(depth, dmin, dmax, tol, radius, ss2, sd2):
    import torch.nn.functional as F

    B, H, W = depth.shape
    ok = (depth >= dmin) & (depth <= dmax) & torch.isfinite(depth)
    pad = F.pad(depth.unsqueeze(1), (1, 1, 1, 1), mode="replicate")[:, 0]
    md = torch.zeros_like(depth)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        nb = pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        nb = torch.where((nb < dmin) | (nb > dmax), depth, nb)
        md = torch.maximum(md, (depth - nb).abs())
    ok = ok & ~(md > tol * depth)
    big = F.pad(depth.unsqueeze(1), (radius,) * 4, value=float("inf"))[:, 0]
    sv, sw = torch.zeros_like(depth), torch.zeros_like(depth)
    for di in range(-radius, radius + 1):
        for dj in range(-radius, radius + 1):
            nb = big[:, radius + di:radius + di + H, radius + dj:radius + dj + W]
            w = torch.exp(torch.tensor(-(di * di + dj * dj) / ss2, device=depth.device)) * torch.exp(-((nb - depth) ** 2) / sd2)
            w = torch.where((nb < dmin) | (nb > dmax), torch.zeros_like(w), w)
            sv = sv + torch.where(w > 0, nb, torch.zeros_like(nb)) * w
            sw = sw + w
    out = torch.where(sw > 1e-8, sv / sw, depth)
    return torch.where(ok, out, torch.zeros_like(out)), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perception_timing.jsonl"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perception_timing needs a GPU"
    from curobo_amd.backends import perception as P
    from curobo_amd.kinematics import Kinematics, KinematicsCfg
    from curobo_amd.perception import FilterDepth, RobotSegmenter
    from curobo_amd.types import CameraObservation, JointState, Pose

    dev = torch.device("cuda:0")
    rows = []
    sizes = [(480, 640)] if args.quick else [(480, 640), (720, 1280)]
    robots = {n: Kinematics(KinematicsCfg.from_packaged(n, device=dev)) for n in ("franka", "unitree_g1")}
    for (H, W) in sizes:
        for B in (1, 4):
            torch.manual_seed(0)
            depth = (1.0 + torch.rand(B, H, W, device=dev)).contiguous()
            K = torch.tensor([[[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1.0]]], device=dev)
            pose = Pose(torch.tensor([[1.2, 0.3, 1.0]], device=dev), torch.tensor([[0.2706, 0.6533, 0.6533, 0.2706]], device=dev))
            obs = CameraObservation(depth_image=depth, intrinsics=K, pose=pose, depth_to_meter=1.0)
            obs.update_projection_rays()
            px = B * H * W
            base = dict(height=H, width=W, batch=B)
            for ksize in (5, 9):
                fd = FilterDepth((H, W), bilateral_kernel_size=ksize, bilateral_sigma_spatial=2.0, bilateral_sigma_depth=0.05, device=str(dev), num_batch=B)
                if args.kernels_only:
                    for _ in range(5):
                        fd(depth)
                    continue
                t, lo, hi = timed(lambda: fd(depth), 50)
                passes = 1 if ksize < 7 else 3
                nbytes = px * (4 + 4 + 1) + (px * 16 if passes == 3 else 0)  # + two scratch images written and read
                te, _, _ = timed(lambda: eager_filter(depth, 0.1, 10.0, fd._flying_tolerance, ksize // 2, fd._sigma_spatial_sq2, fd._sigma_depth_sq2), 3, 3)
                rows.append(dict(base, what=f"filter_{ksize}x{ksize}", launches=passes, seconds=t, seconds_min=lo, seconds_max=hi, bytes=nbytes,
                                 hbm_fraction=nbytes / t / HBM_PEAK, eager_seconds=te, speedup=te / t, taps_per_pixel=ksize * ksize if passes == 1 else 2 * ksize))
            for name, kin in robots.items():
                q = kin.default_joint_position.view(1, -1).contiguous()
                spheres = kin.compute_kinematics(q).robot_spheres.reshape(1, -1, 4).clone()
                S = int(spheres.shape[1])
                mask, out = torch.empty(B, H, W, dtype=torch.uint8, device=dev), torch.empty_like(depth)
                for mode, mname in ((P.MASK_FP32, "fp32"), (P.MASK_BF16_OPS, "bf16_ops")):
                    run = lambda: P.robot_mask(mask, out, depth, obs.projection_rays, pose.position, pose.quaternion, spheres, 0.05, mode)  # noqa: E731
                    if args.kernels_only:
                        for _ in range(5):
                            run()
                        continue
                    t, lo, hi = timed(run, 50)
                    nbytes = px * (4 + 4 + 1) + H * W * 12
                    row = dict(base, what=f"robot_mask_{mname}", robot=name, spheres=S, seconds=t, seconds_min=lo, seconds_max=hi, bytes=nbytes,
                               hbm_fraction=nbytes / t / HBM_PEAK, sphere_tests_per_second=px * S / t, eager_bytes=px * S * 4 * 2 + px * 9)
                    if mode == P.MASK_FP32:
                        if px * S * 4 * 4 < 24e9:
                            te, _, _ = timed(lambda: eager_mask(depth, obs.projection_rays, pose.position, pose.quaternion, spheres, 0.05), 3, 3)
                            row.update(eager_seconds=te, speedup=te / t)
                        else:
                            row.update(eager_seconds=None, eager_note="the pixels x spheres intermediates do not fit a sensible budget")
                    rows.append(row)
                if args.kernels_only:
                    continue
                seg = RobotSegmenter(kin, 0.05, use_cuda_graph=True, ops_dtype=torch.bfloat16)
                js = JointState.from_position(q, kin.joint_names)
                t, lo, hi = timed(lambda: seg.get_robot_mask(obs, js), 50)
                rows.append(dict(base, what="get_robot_mask_graph", robot=name, spheres=S, seconds=t, seconds_min=lo, seconds_max=hi))
    if args.kernels_only:
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
