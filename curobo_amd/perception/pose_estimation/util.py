"""Helpers of the pose detectors (reference pose_estimation/util.py:16-46)."""

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
