"""Helpers of the pose detectors (reference pose_estimation/util.py:16-46, :116-145)."""

import torch

from ...types import CameraObservation


def extract_observed_points(camera_obs: CameraObservation, min_depth: float = 0.1) -> torch.Tensor:
    """the observation's point cloud in the world frame, [N, 3]: pixels of the segmentation (when there is one), finite,
    and with |z| above ``min_depth``"""
    pointcloud_full = camera_obs.get_pointcloud(project_to_pose=True)
    if camera_obs.image_segmentation is not None:
        observed_points = pointcloud_full.view(-1, 3)[(camera_obs.image_segmentation > 0).view(-1)]
    else:
        observed_points = pointcloud_full.view(-1, 3)
    valid_mask = torch.isfinite(observed_points).all(dim=1)
    valid_mask &= observed_points[:, 2].abs() > min_depth
    return observed_points[valid_mask]


def resample_points(points: torch.Tensor, target_count: int, device: torch.device = None) -> torch.Tensor:
    """exactly ``target_count`` of ``points`` [N, 3]: a random subset, or, when there are too few, a random subset of the
    cloud repeated (so points come up more than once)"""
    n_points = len(points)
    if device is None:
        device = points.device
    if n_points < target_count:
        points = points.repeat((target_count // n_points) + 1, 1)
    indices = torch.randperm(len(points), device=device)[:target_count]
    return points[indices]
