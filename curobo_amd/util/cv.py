"""Depth image <-> point cloud helpers (reference ``curobo/_src/geom/cv.py``).  Plain torch: the rays are computed once per
camera; the per-frame work is in ``curobo_amd.perception``."""

from __future__ import annotations

import torch


def get_projection_rays(height: int, width: int, intrinsics_matrix: torch.Tensor, depth_to_meter: float = 0.001) -> torch.Tensor:
    """Rays ``[(u - cx) / fx, (v - cy) / fy, 1] * depth_to_meter`` of every pixel (row-major) for a batch of intrinsics
    (b, 3, 3) -> (b, height * width, 3)"""
    fx, fy = intrinsics_matrix[:, 0:1, 0:1], intrinsics_matrix[:, 1:2, 1:2]
    cx, cy = intrinsics_matrix[:, 0:1, 2:3], intrinsics_matrix[:, 1:2, 2:3]
    dev, b = intrinsics_matrix.device, intrinsics_matrix.shape[0]
    u = torch.arange(width, dtype=torch.float32, device=dev).view(1, 1, width).expand(b, height, width)
    v = torch.arange(height, dtype=torch.float32, device=dev).view(1, height, 1).expand(b, height, width)
    ones = torch.ones((b, height, width), device=dev, dtype=torch.float32)
    rays = torch.stack([(u - cx) / fx, (v - cy) / fy, ones], -1).reshape(b, width * height, 3)
    return rays * depth_to_meter


def project_depth_using_rays(depth_image: torch.Tensor, rays: torch.Tensor, filter_origin: bool = False,
                             depth_threshold: float = 0.01) -> torch.Tensor:
    """depth (b, h, w) x rays (b or 1, h * w, 3) -> points (b, h * w, 3) in the camera frame; ``filter_origin`` zeroes
    depths below ``depth_threshold`` first"""
    if filter_origin:
        depth_image = torch.where(depth_image < depth_threshold, 0, depth_image)
    return depth_image.reshape(depth_image.shape[0], -1, 1).contiguous() * rays
