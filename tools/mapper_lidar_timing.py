"""Times of the mapper's lidar path (csrc/mapper_lidar.hip) at a size a user runs -> <out>/mapper_lidar_timing.jsonl (one line per run).

    python tools/mapper_lidar_timing.py [--out profiles]

One frame of a 64 x 1024 spinning lidar (elevation -0.4 .. 0.3 rad, valid range 0.1 .. 10 m) standing inside the default map of the
reference, 2 m at 5 mm = 400^3 voxels in blocks of 4 (256 MB dense), over the sphere-and-ground scene of tests/mapper_ref.py: the
lidar-mask clear, the marking stage and the voxel stage one by one, and the whole ``integrate`` call.  For scale, one 480 x 640
camera frame into the same map, as tools/mapper_timing.py times it.  Device events around repeated launches after a warm-up, the
median of the rounds; every launch is repeatable (marking sets bytes that are already set; the voxel stage adds to the sums, which
changes no launch's work).  Beside each time the bytes the stage has to move (computed from the shapes and the visible-block count;
the definitions are in the code) and what share of the 6.29 TB/s a float4 copy reaches on this part that is: the voxel stage does
two double-precision atan2 and a square root per voxel and sensor, so expect it to be bound by arithmetic, not by memory.  For the
kernels' own times run this under ``rocprofv3 --kernel-trace --stats`` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import mapper_lidar_ref as LR  # noqa: E402  (the analytic range image of a sphere over a ground plane)
import mapper_ref as R  # noqa: E402
from curobo_amd.backends import mapper as B  # noqa: E402
from curobo_amd.perception.mapper import Mapper, MapperCfg, MapperLidarCfg  # noqa: E402
from curobo_amd.types import CameraObservation, LidarObservation, Pose  # noqa: E402
from mapper_timing import DEV, stage, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mapper_lidar_timing needs a GPU"
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    H, W, LH, LW = 480, 640, 64, 1024
    cfg = MapperCfg(extent_meters_xyz=(2.0, 2.0, 2.0), voxel_size=0.005, image_height=H, image_width=W, esdf_voxel_size=2.0 / 128,
                    extent_esdf_meters_xyz=(2.0, 2.0, 2.0))
    result = {"when": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "map_voxels": [int(v) for v in cfg.grid_shape]}

    # the lidar frame
    m = Mapper(cfg, lidar=MapperLidarCfg(num_sensors=1, image_height=LH, image_width=LW))
    p, ts = m.tsdf.params, m.tsdf
    eye, quat = np.array([0.7, -0.55, 0.2], np.float32), np.array([np.cos(0.3), 0.0, 0.0, np.sin(0.3)], np.float32)
    elev, valid = np.array([-0.4, 0.3], np.float32), np.array([0.1, 10.0], np.float32)
    rng = LR.render_range(eye, quat, LH, LW, float(elev[0]), float(elev[1]))
    obs = LidarObservation(range_image=t(rng[None]), pose=Pose(t(eye[None]), t(quat[None])), valid_range_m=t(valid[None]),
                           elevation_range_rad=t(elev[None]))
    lidar = m._lidar_tensors(obs)
    m.integrate(obs)
    torch.cuda.synchronize()
    visible, blocks, bs3 = int(ts.lidar_frame_visible[: p.n_blocks].sum().item()), p.n_blocks, p.block_voxels
    lanes = LH * LW * p.num_samples
    vs = float(cfg.voxel_size)
    guards = (m.lidar_config.linear_interpolation_max_allowable_difference_vox * vs, m.lidar_config.nearest_interpolation_max_allowable_dist_to_ray_vox * vs)
    result["lidar_frame"] = {
        "image": [LH, LW], "returns": round(float((rng > 0).mean()), 4), "blocks": blocks, "visible_blocks": visible,
        "workgroups_that_return_at_once": round(1.0 - visible / blocks, 4), "samples_per_pixel": int(p.num_samples),
        # the mask's bytes written
        "clear_mask": stage(timed(lambda: B.mapper_clear_mask(ts.lidar_frame_visible)), blocks),
        # the range image read once per sample lane group (cached after the first), three bytes stored per live lane at most
        "mark": stage(timed(lambda: B.mapper_lidar_mark_blocks(ts.lidar_frame_visible, ts.frame_visible, ts.block_visible, *lidar, p)), LH * LW * 4 + lanes * 4),
        # every mask byte read, the visible blocks' words read and written, up to five pixels read per voxel (cached: the image is 256 KB)
        "voxels": stage(timed(lambda: B.mapper_lidar_integrate(ts.block_data, ts.lidar_frame_visible, *lidar, p, *guards)), blocks + visible * bs3 * 8),
        "whole_call": {"ms": round(timed(lambda: m.integrate(obs)), 4)}}
    del m, ts
    torch.cuda.empty_cache()

    # for scale: one camera frame into the same map
    K = np.array([[520.0, 0, 320.3], [0, 520.0, 239.6], [0, 0, 1]], np.float32)
    ceye = np.array([1.0, -0.6, 0.5], np.float32)
    cquat = R.look_at(ceye, (0.0, 0.0, -0.05), 0.3).astype(np.float32)
    cobs = CameraObservation(depth_image=t(R.render_depth(K, ceye, cquat, H, W)[None]), intrinsics=t(K[None]), pose=Pose(t(ceye[None]), t(cquat[None])))
    m = Mapper(cfg)
    p, ts = m.tsdf.params, m.tsdf
    d, k, pos, q = m._camera_tensors(cobs)
    m.integrate(cobs)
    torch.cuda.synchronize()
    visible = m.get_stats()["last_frame_blocks"]
    result["camera_frame"] = {
        "image": [H, W], "visible_blocks": visible,
        "mark": stage(timed(lambda: B.mapper_mark_blocks(ts.frame_visible, ts.block_visible, d, k, pos, q, p)), H * W * 4 + H * W * p.num_samples * 2),
        "voxels": stage(timed(lambda: B.mapper_integrate(ts.block_data, ts.frame_visible, d, k, pos, q, p)), blocks + visible * bs3 * 8),
        "whole_call": {"ms": round(timed(lambda: m.integrate(cobs)), 4)}}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "mapper_lidar_timing.jsonl"), "a") as fh:
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
