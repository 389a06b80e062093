"""Times of the depth mapper (csrc/mapper.hip) at the sizes a user runs -> <out>/mapper_timing.jsonl (one line per run).

    python tools/mapper_timing.py [--out profiles] [--sections map raycast decay]

integrate: one 480 x 640 frame into the default map of the reference, 2 m at 5 mm = 400^3 voxels in blocks of 4 (256 MB dense),
split into the frame-mask clear, the marking stage and the voxel stage.  compute_esdf: the captured chain at 128^3 and 256^3
cells over the same map, and its five launches one by one.  Device events around repeated launches after a warm-up, the median
of the rounds.  extract_mesh: the whole call on that map after its one frame, by the host's clock (it reads three totals back, so
the call ends synchronised), without and with two refinement steps.  Beside each time the bytes the stage has to move (computed from the shapes and the visible-block count; the
definitions are in the code) and what share of the 6.29 TB/s a float4 copy reaches on this part that is.

raycast (csrc/mapper_raycast.hip): a 640 x 480 view of a 256^3 map of 1 cm voxels after 24 frames from around the scene (about a
tenth of the blocks visible; the share is in the output): one launch of each form of the render, one alignment evaluation at the
refiner's default n_points = 92160 (stride 1 at this image: every pixel), and a whole ``refine_pose`` of 100 iterations by the
host's clock.

decay (csrc/mapper.hip, curobo_hip_mapper_decay): a 2 m cube at 1 cm in blocks of 4 after six frames from around the scene: the
launch without and with one camera's frustum test, and beside it the torch formulation the reference uses on the same tensors
(``mul_`` by a per-block fp16 factor, the fp32 block sum, a mask update).  Every factor is 1, so that the map is the same at every
repetition.  The launch has to move 8 B per voxel of a visible block and 1 B per block; the torch chain touches every block.  For
the kernel's own time run this section under ``rocprofv3 --kernel-trace --stats`` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mapper_ref as R  # noqa: E402  (the analytic depth image of a sphere over a ground plane)
from curobo_amd.backends import mapper as B  # noqa: E402
from curobo_amd.backends import perception as BP  # noqa: E402
from curobo_amd.perception.mapper import (BlockSparseRaycastPoseRefiner, BlockSparseRaycastRefinerCfg, BlockSparseTSDFRenderer, Mapper,  # noqa: E402
                                          MapperCfg)
from curobo_amd.types import CameraObservation, Pose  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate (8.0 TB/s on paper)


def timed(fn, reps=20, rounds=5, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def wall_ms(fn, reps=5):
    """a call that synchronises by itself: the host's clock, the median of ``reps`` calls after one"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def stage(ms: float, nbytes: float) -> dict:
    return {"ms": round(ms, 4), "MB": round(nbytes / 1e6, 2), "share_of_hbm": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}


def raycast_times(H, W, K) -> dict:
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    cfg = MapperCfg(extent_meters_xyz=(2.56, 2.56, 2.56), voxel_size=0.01, image_height=H, image_width=W, esdf_voxel_size=0.04,
                    extent_esdf_meters_xyz=(2.56, 2.56, 2.56), truncation_distance=0.08)
    m = Mapper(cfg)
    # four rings of six eyes, each looking a little past the sphere, so that the frames also cover the ground around it
    eyes = [(1.2 * np.cos(a), 1.2 * np.sin(a), h) for h in (0.35, 0.65, 0.95, 1.3) for a in np.arange(6) * (np.pi / 3) + h]
    for eye in eyes:
        eye = np.asarray(eye, np.float32)
        quat = R.look_at(eye, (-0.25 * eye[0], -0.25 * eye[1], -0.05), 0.2).astype(np.float32)
        m.integrate(CameraObservation(depth_image=t(R.render_depth(K, eye, quat, H, W)[None]), intrinsics=t(K[None]), pose=Pose(t(eye[None]), t(quat[None]))))
    stats = m.get_stats()
    eye = np.array([0.8, -0.9, 0.6], np.float32)  # a view that integrated nothing
    quat = R.look_at(eye, (0.0, 0.0, -0.05), -0.1).astype(np.float32)
    pose = Pose(t(eye[None]), t(quat[None]))
    out = {"map_voxels": [int(v) for v in cfg.grid_shape], "blocks": stats["total_blocks"], "visible_share": round(stats["visible_blocks"] / stats["total_blocks"], 4)}
    ts, n = m.tsdf, H * W
    for name, accelerated in (("render_plain", False), ("render_accelerated", True)):
        r = BlockSparseTSDFRenderer(m, use_block_acceleration=accelerated)
        depth, _, valid = r.render(t(K), pose, (H, W))
        c = r.config
        launch = lambda r=r, c=c, a=accelerated: B.mapper_raycast(r._hit_points[:n], r._hit_normals[:n], r._hit_depths[:n], r._hit_mask[:n],  # noqa: E731
                                                                  r.intrinsics_matrix, r.cam_position, r.cam_quaternion, ts.block_data, ts.block_visible,
                                                                  ts.params, c.minimum_tsdf_weight, c.depth_minimum_distance, c.depth_maximum_distance,
                                                                  (H, W), a)
        out[name] = {"ms": round(timed(launch, reps=5, rounds=3, warmup=1), 4), "hit_share": round(float(valid.float().mean()), 4)}
    z = BlockSparseTSDFRenderer(m).render_depth(t(K), pose, (H, W), z_depth=True).clone()
    rcfg = BlockSparseRaycastRefinerCfg(minimum_tsdf_weight=cfg.minimum_tsdf_weight)
    refiner = BlockSparseRaycastPoseRefiner(m, rcfg)
    off = Pose(t((eye + np.float32([0.02, -0.02, 0.01]))[None]), t(quat[None]))
    _, error, iterations = refiner.refine_pose(z, t(K), off)
    run = refiner._runs[(H, W)]
    out["align_evaluation"] = {"ms": round(timed(lambda: refiner._evaluate(run), reps=10, rounds=3, warmup=1), 4), "samples": run.n_samples,
                               "rows": BP.pose_sdf_ws_bytes(run.n_samples) // 128}
    out["lm_step"] = {"ms": round(timed(lambda: refiner._step(run, BP.POSE_LM_UPDATE), reps=10, rounds=3, warmup=1), 4)}
    out["refine_pose"] = {"ms": round(wall_ms(lambda: refiner.refine_pose(z, t(K), off), reps=3), 3), "iterations": iterations, "final_error": round(error, 6)}
    return out


def decay_times(H, W, K) -> dict:
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    cfg = MapperCfg(extent_meters_xyz=(2.0, 2.0, 2.0), voxel_size=0.01, image_height=H, image_width=W, esdf_voxel_size=0.04,
                    extent_esdf_meters_xyz=(2.0, 2.0, 2.0), truncation_distance=0.08)
    m = Mapper(cfg)
    cams = []
    for a in np.arange(6) * (np.pi / 3):
        eye = np.array([1.2 * np.cos(a), 1.2 * np.sin(a), 0.5], np.float32)
        quat = R.look_at(eye, (-0.25 * eye[0], -0.25 * eye[1], -0.05), 0.2).astype(np.float32)
        cams.append((t(K[None]), t(eye[None]), t(quat[None])))
        m.integrate(CameraObservation(depth_image=t(R.render_depth(K, eye, quat, H, W)[None]), intrinsics=cams[-1][0], pose=Pose(*cams[-1][1:])))
    ts, p = m.tsdf, m.tsdf.params
    n, bs3, thr = p.n_blocks, p.block_voxels, B.decay_empty_threshold(p.block_size)
    gone = m.recycle_empty_blocks()  # (blocks that were marked and received no weight: afterwards every launch below keeps the map as it is)
    visible = m.get_stats()["visible_blocks"]
    nbytes = visible * bs3 * 8 + n
    plain = lambda: B.mapper_decay(ts.block_data, ts.block_visible, ts.block_recycled, p, 1.0, 1.0, thr)  # noqa: E731
    frustum = lambda: B.mapper_decay(ts.block_data, ts.block_visible, ts.block_recycled, p, 1.0, 1.0, thr, *cams[0], image_shape=(H, W))  # noqa: E731
    factor = torch.ones(n, dtype=torch.float16, device=DEV)
    sums = torch.zeros(n, dtype=torch.float32, device=DEV)

    def torch_chain():
        ts.block_data.mul_(factor.view(n, 1, 1))
        sums.copy_(ts.block_data[:, :, 1].sum(dim=1, dtype=torch.float32))
        ts.block_visible[:n].mul_(~((sums < thr) & (ts.block_visible[:n] != 0)))

    before = ts.block_data.clone()
    out = {"map_voxels": [int(v) for v in cfg.grid_shape], "blocks": n, "visible_blocks": visible, "recycled_as_never_weighted": gone,
           "launch": stage(timed(plain), nbytes), "launch_one_camera": stage(timed(frustum), nbytes),
           # the torch chain reads and writes every word of the dense map, then reads every weight again
           "torch_chain": stage(timed(torch_chain), n * bs3 * 10 + n * 6)}
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int16), ts.block_data.view(torch.int16)) and m.get_stats()["visible_blocks"] == visible
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sections", nargs="+", choices=["map", "raycast", "decay"], default=["map", "raycast"],
                    help="map: integrate, compute_esdf, extract_mesh; raycast: render, alignment, refine_pose; decay: the decay launch")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mapper_timing needs a GPU"
    H, W = 480, 640
    K = np.array([[520.0, 0, 320.3], [0, 520.0, 239.6], [0, 0, 1]], np.float32)
    eye = np.array([1.0, -0.6, 0.5], np.float32)
    quat = R.look_at(eye, (0.0, 0.0, -0.05), 0.3).astype(np.float32)
    depth = R.render_depth(K, eye, quat, H, W)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    obs = CameraObservation(depth_image=t(depth[None]), intrinsics=t(K[None]), pose=Pose(t(eye[None]), t(quat[None])))
    result = {"when": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "image": [H, W]}
    for n_esdf in (128, 256) if "map" in args.sections else ():
        cfg = MapperCfg(extent_meters_xyz=(2.0, 2.0, 2.0), voxel_size=0.005, image_height=H, image_width=W, esdf_voxel_size=2.0 / n_esdf,
                        extent_esdf_meters_xyz=(2.0, 2.0, 2.0))
        m = Mapper(cfg)
        p, ts = m.tsdf.params, m.tsdf
        d, k, pos, q = m._camera_tensors(obs)
        m.integrate(obs)
        torch.cuda.synchronize()
        stats = m.get_stats()
        visible, blocks, bs3 = stats["last_frame_blocks"], p.n_blocks, p.block_voxels
        if n_esdf == 128:
            lanes = H * W * p.num_samples
            result["integrate"] = {
                "map_voxels": [int(v) for v in cfg.grid_shape], "blocks": blocks, "visible_blocks": visible,
                "workgroups_that_return_at_once": round(1.0 - visible / blocks, 4), "samples_per_pixel": int(p.num_samples),
                # the mask's bytes written
                "clear_mask": stage(timed(lambda: B.mapper_clear_mask(ts.frame_visible)), blocks),
                # the depth image read once per sample lane group (cached after the first), one byte stored per live lane at most
                "mark": stage(timed(lambda: B.mapper_mark_blocks(ts.frame_visible, ts.block_visible, d, k, pos, q, p)), H * W * 4 + lanes * 2),
                # every mask byte read, the visible blocks' words read and written
                "voxels": stage(timed(lambda: B.mapper_integrate(ts.block_data, ts.frame_visible, d, k, pos, q, p)), blocks + visible * bs3 * 8),
                "whole_call": {"ms": round(timed(lambda: m.integrate(obs)), 4)}}
            vertices, triangles, _, _ = m.extract_mesh_tensors()
            result["extract_mesh"] = {"visible_blocks": stats["visible_blocks"], "vertices": int(vertices.shape[0]), "triangles": int(triangles.shape[0]),
                                      "ms": round(wall_ms(lambda: m.extract_mesh_tensors()), 3),
                                      "ms_two_refinement_steps": round(wall_ms(lambda: m.extract_mesh_tensors(refine_iterations=2)), 3),
                                      "ms_surface_only": round(wall_ms(lambda: m.extract_mesh_tensors(surface_only=True)), 3)}
        shape = m.esdf_grid_shape
        cells = int(np.prod(shape))
        m.compute_esdf()
        torch.cuda.synchronize()
        o, v = m._esdf_origin, m._esdf_voxel_size
        entry = {"cells": list(shape), "captured_chain": {"ms": round(timed(lambda: m._graph.replay()), 4)},
                 "whole_call": {"ms": round(timed(lambda: m.compute_esdf()), 4)},
                 # a site word written per cell; the 7 probes of a cell read TSDF words, at most the whole dense map
                 "seed": stage(timed(lambda: B.mapper_esdf_seed(m._sites, ts.block_data, ts.block_visible, o, v, p, shape)),
                               cells * 4 + min(cells * 7 * 4, cfg.dense_bytes)),
                 # a pass reads every site word, writes every site word and gathers one
                 **{f"pass_{name}": stage(timed(lambda a=axis: B.mapper_edt_pass(m._sites_scratch, m._sites, shape, a)), cells * 12)
                    for name, axis in (("z", 2), ("y", 1), ("x", 0))},
                 # a site word and one TSDF word read, an fp16 written
                 "distance": stage(timed(lambda: B.mapper_esdf_distance(m._dist_field, m._sites_scratch, ts.block_data, ts.block_visible, o, v, p, shape)),
                                   cells * 10)}
        result[f"esdf_{n_esdf}"] = entry
        del m
        torch.cuda.empty_cache()
    if "raycast" in args.sections:
        result["raycast"] = raycast_times(H, W, K)
    if "decay" in args.sections:
        result["decay"] = decay_times(H, W, K)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "mapper_timing.jsonl"), "a") as fh:
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
