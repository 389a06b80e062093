"""Weight decay and block recycling of the mapper's TSDF: the module functions of the reference's ``kernel/wp_decay.py`` over
``DenseTSDF``, one launch of ``curobo_hip_mapper_decay`` each, or of ``curobo_hip_mapper_decay_sensors`` where lidars have a
frustum too (``csrc/mapper.hip``).

The reference multiplies the whole pool with torch (``block_data.mul_``), sums every block's weights and launches a recycle kernel
over the sums; here one launch does the three per ever-visible block and reads nothing of the others.  Its two paths round the
factor differently and both are kept bit for bit: the uniform path (``frustum_decay >= 1``, ``decay_and_recycle``) multiplies the
fp16 words by the factor as a float32, the frustum path by a per-block factor that is itself fp16 (``storage.py:390``): the host
rounds, the launch multiplies in fp32 and rounds to fp16.  "Allocated" is the byte ``block_visible``: a recycled block's byte
and words become 0, so a later frame that marks it again integrates into an empty block, as the reference's re-allocation does
(``builder_hash.py:474-492``); ``frame_visible`` is not touched."""

from __future__ import annotations

import copy
from typing import Optional, Sequence

import torch

from ...backends import mapper as B


def _f32(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32).item())


def _f16(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float16).item())


def check_factor(name: str, value: float) -> float:
    """a decay factor of the mapper's own interface: in (0, 1]"""
    if not 0.0 < float(value) <= 1.0:
        raise ValueError(f"{name} must be in (0, 1]: {value}")
    return float(value)


def recycled_count(tsdf) -> int:
    """how many blocks the last decay launch recycled (one read back to the host)"""
    return int(tsdf.block_recycled[: tsdf.n_blocks].sum().item())


def _launch(tsdf, factor_outside: float, factor_inside: float, params=None, cameras=(None, None, None), image_shape=(0, 0)) -> None:
    params = tsdf.params if params is None else params
    with torch.cuda.device(tsdf.block_data.device):
        B.mapper_decay(tsdf.block_data, tsdf.block_visible, tsdf.block_recycled, params, factor_outside, factor_inside,
                       B.decay_empty_threshold(params.block_size), *cameras, image_shape=image_shape)


def _launch_sensors(tsdf, factor_outside: float, factor_inside: float, params, cameras, image_shape, lidars, lidar_height: int) -> None:
    with torch.cuda.device(tsdf.block_data.device):
        B.mapper_decay_sensors(tsdf.block_data, tsdf.block_visible, tsdf.block_recycled, params, factor_outside, factor_inside,
                               B.decay_empty_threshold(params.block_size), *cameras, image_shape, *lidars, lidar_height)


def decay_and_recycle(tsdf, decay_factor: float = 0.95) -> int:
    """every voxel's pair times ``decay_factor`` (left alone when it is >= 1), then every block whose weights sum to less than
    ``0.01 block_size^3 / 8^3`` recycled; returns how many were (a read back to the host: not for a captured graph).
    Reference ``wp_decay.py:28-59``."""
    if not float(decay_factor) > 0.0:
        raise ValueError(f"decay_factor must be positive: {decay_factor}")
    factor = _f32(decay_factor) if decay_factor < 1.0 else 1.0  # fp16 tensor times a Python scalar: the scalar as float32
    _launch(tsdf, factor, factor)
    return recycled_count(tsdf)


def decay_frustum_aware_multi_camera(tsdf, intrinsics: torch.Tensor, cam_positions: torch.Tensor, cam_quaternions: torch.Tensor,
                                     img_shape: Sequence[int], depth_minimum_distance: float = 0.1, depth_maximum_distance: float = 10.0,
                                     time_decay: float = 1.0, frustum_decay: float = 0.5, num_blocks: Optional[int] = None) -> None:
    """``time_decay`` for every ever-visible block, ``time_decay frustum_decay`` for those in the union of the cameras' frusta
    (``intrinsics`` [n, 3, 3], ``cam_positions`` [n, 3], ``cam_quaternions`` [n, 4] wxyz, ``img_shape`` (H, W), float32 on the
    map's device; the depth images are not looked at), then the recycling of ``decay_and_recycle``.  With ``frustum_decay >= 1``
    no frustum is tested and the factor is rounded as the uniform path rounds it.  ``num_blocks`` (the reference's slice of its
    pool) is accepted and has no effect.  Nothing is read back: ``tsdf.block_recycled`` says what was recycled.
    Reference ``wp_decay.py:111-149, 294-331``."""
    if not (float(time_decay) > 0.0 and float(frustum_decay) > 0.0):
        raise ValueError(f"time_decay and frustum_decay must be positive: {time_decay}, {frustum_decay}")
    if frustum_decay >= 1.0:
        factor = _f32(time_decay) if time_decay < 1.0 else 1.0
        _launch(tsdf, factor, factor)
        return
    if not float(time_decay) <= 1.0:
        raise ValueError(f"time_decay must be <= 1 on the frustum path: {time_decay}")
    params = copy.copy(tsdf.params)  # the frustum test's depth range is this call's, not the integration's
    params.depth_min, params.depth_max = float(depth_minimum_distance), float(depth_maximum_distance)
    f32 = dict(device=tsdf.block_data.device, dtype=torch.float32)
    cameras = (intrinsics.to(**f32).reshape(-1, 3, 3).contiguous(), cam_positions.to(**f32).reshape(-1, 3).contiguous(),
               cam_quaternions.to(**f32).reshape(-1, 4).contiguous())
    # the per-block factor tensor is fp16: both values rounded on the fill, the in-frustum one from the product in double
    _launch(tsdf, _f16(time_decay), _f16(float(time_decay) * float(frustum_decay)), params, cameras,
            (int(img_shape[0]), int(img_shape[1])))


def decay_frustum_aware_multi_sensor(tsdf, *, camera_intrinsics: Optional[torch.Tensor] = None, camera_positions: Optional[torch.Tensor] = None,
                                     camera_quaternions: Optional[torch.Tensor] = None, camera_img_shape: Optional[Sequence[int]] = None,
                                     camera_depth_minimum_distance: float = 0.1, camera_depth_maximum_distance: float = 10.0,
                                     lidar_positions: Optional[torch.Tensor] = None, lidar_quaternions: Optional[torch.Tensor] = None,
                                     lidar_valid_range_m: Optional[torch.Tensor] = None, lidar_elevation_range_rad: Optional[torch.Tensor] = None,
                                     lidar_img_shape: Optional[Sequence[int]] = None, time_decay: float = 1.0, frustum_decay: float = 0.5,
                                     num_blocks: Optional[int] = None) -> None:
    """``decay_frustum_aware_multi_camera`` over the union of the frusta of cameras AND lidars, either of which may be left out:
    ``lidar_positions`` [n, 3], ``lidar_quaternions`` [n, 4] wxyz, ``lidar_valid_range_m`` [n, 2], ``lidar_elevation_range_rad``
    [n, 2], ``lidar_img_shape`` (H, W) of the range images (H == 1: a planar scan, tested against its one elevation), float32 on
    the map's device.  A lidar's frustum is its range band and elevation band over every azimuth; neither depth nor range images
    are looked at.  One launch of ``curobo_hip_mapper_decay_sensors``; the factors are rounded as the camera path rounds them.
    Reference ``wp_decay.py:152-291``, ``builder_decay.py:217-313``."""
    if not (float(time_decay) > 0.0 and float(frustum_decay) > 0.0):
        raise ValueError(f"time_decay and frustum_decay must be positive: {time_decay}, {frustum_decay}")
    if frustum_decay >= 1.0:
        factor = _f32(time_decay) if time_decay < 1.0 else 1.0
        _launch(tsdf, factor, factor)
        return
    if not float(time_decay) <= 1.0:
        raise ValueError(f"time_decay must be <= 1 on the frustum path: {time_decay}")
    f32 = dict(device=tsdf.block_data.device, dtype=torch.float32)
    params = copy.copy(tsdf.params)  # the frustum test's depth range is this call's, not the integration's
    cameras, image_shape = (None, None, None), (0, 0)
    if camera_intrinsics is not None:
        if camera_positions is None or camera_quaternions is None or camera_img_shape is None:
            raise ValueError("camera_intrinsics requires camera_positions, camera_quaternions, and camera_img_shape.")
        params.depth_min, params.depth_max = float(camera_depth_minimum_distance), float(camera_depth_maximum_distance)
        cameras = (camera_intrinsics.to(**f32).reshape(-1, 3, 3).contiguous(), camera_positions.to(**f32).reshape(-1, 3).contiguous(),
                   camera_quaternions.to(**f32).reshape(-1, 4).contiguous())
        image_shape = (int(camera_img_shape[0]), int(camera_img_shape[1]))
    lidars, lidar_height = (None, None, None, None), 0
    if lidar_positions is not None:
        if lidar_quaternions is None or lidar_valid_range_m is None or lidar_elevation_range_rad is None or lidar_img_shape is None:
            raise ValueError("lidar_positions requires lidar_quaternions, lidar_valid_range_m, lidar_elevation_range_rad, and lidar_img_shape.")
        lidar_height = int(lidar_img_shape[0])
        if lidar_height <= 0:
            raise ValueError(f"lidar_img_shape height must be positive, got {lidar_height}.")
        lidars = (lidar_positions.to(**f32).reshape(-1, 3).contiguous(), lidar_quaternions.to(**f32).reshape(-1, 4).contiguous(),
                  lidar_valid_range_m.to(**f32).reshape(-1, 2).contiguous(), lidar_elevation_range_rad.to(**f32).reshape(-1, 2).contiguous())
    # the per-block factor tensor is fp16: both values rounded on the fill, the in-frustum one from the product in double
    _launch_sensors(tsdf, _f16(time_decay), _f16(float(time_decay) * float(frustum_decay)), params, cameras, image_shape, lidars, lidar_height)
