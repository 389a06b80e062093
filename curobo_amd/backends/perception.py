"""HIP backend of ``curobo_amd.perception`` (``csrc/perception.hip``: filter_depth_kernel and robot_mask_kernel).  Same
conventions as the other backends: pre-allocated tensors in, mutated in place, current stream."""

from __future__ import annotations

from typing import Optional

import torch

from .._lib import check, current_stream, load, ptr

#: arithmetic modes of ``robot_mask`` (``bf16_ops`` argument of ``curobo_hip_robot_mask``)
MASK_FP32, MASK_BF16_OPS = 0, 1


def _require(t: Optional[torch.Tensor], name: str, dtype: torch.dtype, like: Optional[torch.Tensor] = None) -> None:
    if t is None:
        return
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor, got {t.dtype} with strides {tuple(t.stride())}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, expected {like.device}")


def filter_depth(depth_out: torch.Tensor, valid_mask_out: torch.Tensor, depth_in: torch.Tensor, temp_a: Optional[torch.Tensor],
                 temp_b: Optional[torch.Tensor], depth_minimum_distance: float, depth_maximum_distance: float,
                 enable_flying_pixel: bool, flying_tolerance: float, bilateral_kernel_size: int, sigma_spatial_sq2: float,
                 sigma_depth_sq2: float) -> None:
    """``curobo_hip_filter_depth``: (B, H, W) fp32 depth -> depth_out fp32 (rejected pixels 0), valid_mask_out uint8.
    ``bilateral_kernel_size`` 0 switches smoothing off; sizes >= 7 need the two (B, H, W) fp32 scratch images."""
    if depth_in.dim() != 3:
        raise ValueError(f"filter_depth: depth must be (B, H, W), got {tuple(depth_in.shape)}")
    _require(depth_in, "depth_in", torch.float32)
    _require(depth_out, "depth_out", torch.float32, depth_in)
    _require(valid_mask_out, "valid_mask_out", torch.uint8, depth_in)
    for name, t in (("depth_out", depth_out), ("valid_mask_out", valid_mask_out), ("temp_a", temp_a), ("temp_b", temp_b)):
        if t is not None and tuple(t.shape) != tuple(depth_in.shape):
            raise ValueError(f"filter_depth: {name} has shape {tuple(t.shape)}, depth {tuple(depth_in.shape)}")
    _require(temp_a, "temp_a", torch.float32, depth_in)
    _require(temp_b, "temp_b", torch.float32, depth_in)
    B, H, W = (int(v) for v in depth_in.shape)
    check(load().curobo_hip_filter_depth(
        ptr(depth_out), ptr(valid_mask_out), ptr(depth_in), ptr(temp_a), ptr(temp_b), B, H, W, float(depth_minimum_distance),
        float(depth_maximum_distance), int(bool(enable_flying_pixel)), float(flying_tolerance), int(bilateral_kernel_size),
        float(sigma_spatial_sq2), float(sigma_depth_sq2), current_stream(depth_in)))


def robot_mask(mask_out: torch.Tensor, depth_out: torch.Tensor, depth: torch.Tensor, projection_rays: torch.Tensor,
               camera_position: torch.Tensor, camera_quaternion: torch.Tensor, robot_spheres: torch.Tensor,
               distance_threshold: float, mode: int = MASK_FP32) -> None:
    """``curobo_hip_robot_mask``: depth (B, H, W), projection_rays (B or 1, H W, 3), camera pose (B or 1, 3) / (B or 1, 4) wxyz,
    robot_spheres (B or 1, S, 4) -> mask_out uint8 (B, H, W), depth_out = depth with the robot's pixels set to 0."""
    if depth.dim() != 3:
        raise ValueError(f"robot_mask: depth must be (B, H, W), got {tuple(depth.shape)}")
    B, H, W = (int(v) for v in depth.shape)
    _require(depth, "depth", torch.float32)
    for name, t in (("depth_out", depth_out), ("projection_rays", projection_rays), ("camera_position", camera_position),
                    ("camera_quaternion", camera_quaternion), ("robot_spheres", robot_spheres)):
        _require(t, name, torch.float32, depth)
    _require(mask_out, "mask_out", torch.uint8, depth)
    if tuple(mask_out.shape) != (B, H, W) or tuple(depth_out.shape) != (B, H, W):
        raise ValueError(f"robot_mask: mask_out / depth_out must have shape {(B, H, W)}")
    if projection_rays.dim() != 3 or tuple(projection_rays.shape[1:]) != (H * W, 3):
        raise ValueError(f"robot_mask: projection_rays must be (B or 1, {H * W}, 3), got {tuple(projection_rays.shape)}")
    pos, quat = camera_position.reshape(-1, 3), camera_quaternion.reshape(-1, 4)
    if pos.shape[0] != quat.shape[0]:
        raise ValueError("robot_mask: camera position and quaternion batches differ")
    if robot_spheres.dim() != 3 or robot_spheres.shape[-1] != 4:
        raise ValueError(f"robot_mask: robot_spheres must be (B or 1, S, 4), got {tuple(robot_spheres.shape)}")
    check(load().curobo_hip_robot_mask(
        ptr(mask_out), ptr(depth_out), ptr(depth), ptr(projection_rays), ptr(pos), ptr(quat), ptr(robot_spheres), B, H, W,
        int(robot_spheres.shape[1]), int(projection_rays.shape[0]), int(pos.shape[0]), int(robot_spheres.shape[0]),
        float(distance_threshold), int(mode), current_stream(depth)))
