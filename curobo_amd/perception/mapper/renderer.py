"""``BlockSparseTSDFRenderer``: depth, normal and shaded images of the mapper's TSDF from any camera pose, by one HIP launch
per image (``curobo_hip_mapper_raycast``, ``csrc/mapper_raycast.hip``; reference ``perception/mapper/renderer.py``).

The depth image is what the reference returns: the RANGE along each pixel's ray (its ``z_depth = hit_t * ray_cam_z`` multiplies by
the un-normalised 1.0, ``builder_raycast.py:564``), not the depth along the camera's axis.  ``z_depth=True`` -- this project's
addition -- returns range times the z of the normalised ray instead, which is what a depth camera measures and what
``Mapper.integrate`` and the pose refiner read.

``use_block_acceleration`` selects the reference's second kernel, which jumps over blocks no frame has seen.  It samples at other
points along the ray than the plain march and so returns slightly different depths: two contracts, not one with a fast path.

This mapper has no colour channel: the colour images are all zero (the rule of ``Mapper.extract_mesh``'s ``vertex_colors``) and
``render_shaded`` shades grey; ``use_color=True`` raises.

The output buffers are kept and grown as in the reference: the tensors ``render`` returns are VIEWS of them, rewritten by the
next call on this renderer.  Clone what has to outlive it."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ...backends import mapper as B
from ...types import Pose


@dataclass
class BlockSparseTSDFRendererCfg:
    """``depth_minimum_distance`` / ``depth_maximum_distance``: the range marched along a ray, metres; ``minimum_tsdf_weight``: a
    voxel is read when its weight is at least this; ``use_block_acceleration``: skip blocks never seen (reference renderer.py:39-58)"""

    depth_minimum_distance: float = 0.2
    depth_maximum_distance: float = 15.0
    minimum_tsdf_weight: float = 0.2
    use_block_acceleration: bool = True


class BlockSparseTSDFRenderer:
    """``BlockSparseTSDFRenderer(mapper)``; depth range and minimum weight are the mapper's configuration's, as the reference takes
    them from its integrator."""

    def __init__(self, mapper, use_block_acceleration: bool = True):
        self.mapper = mapper
        c = mapper.config
        self.config = BlockSparseTSDFRendererCfg(depth_minimum_distance=c.depth_minimum_distance, depth_maximum_distance=c.depth_maximum_distance,
                                                 minimum_tsdf_weight=c.minimum_tsdf_weight, use_block_acceleration=use_block_acceleration)
        self.device = torch.device(c.device)
        self._buffer_size = 0
        self._hit_points = self._hit_normals = self._hit_colors = self._hit_depths = self._hit_mask = None
        # the camera the launch reads, on the device
        self.cam_position = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.cam_quaternion = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.intrinsics_matrix = torch.zeros((3, 3), dtype=torch.float32, device=self.device)

    def _ensure_buffers(self, n_pixels: int) -> None:
        if self._buffer_size >= n_pixels:
            return
        f32 = dict(dtype=torch.float32, device=self.device)
        self._hit_points, self._hit_normals = torch.zeros((n_pixels, 3), **f32), torch.zeros((n_pixels, 3), **f32)
        self._hit_colors = torch.zeros((n_pixels, 3), dtype=torch.uint8, device=self.device)  # no colour channel: stays zero
        self._hit_depths = torch.zeros(n_pixels, **f32)
        self._hit_mask = torch.zeros(n_pixels, dtype=torch.uint8, device=self.device)
        self._buffer_size = n_pixels

    def _extract_pose(self, pose: Pose) -> None:
        position, quaternion = pose.position.reshape(-1), pose.quaternion.reshape(-1)
        if position.numel() != 3 or quaternion.numel() != 4:
            raise ValueError(f"pose must be one camera pose, got position {tuple(pose.position.shape)} and quaternion {tuple(pose.quaternion.shape)}")
        self.cam_position.copy_(position.to(self.device, torch.float32))
        self.cam_quaternion.copy_(quaternion.to(self.device, torch.float32))

    def render(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int], *, z_depth: bool = False):
        """``(depth [H, W] float32, 0 where nothing was hit; normals [H, W, 3] in the world frame; valid [H, W] bool)``.
        ``intrinsics`` [3, 3] or [fx, fy, cx, cy]; ``pose`` the camera in the world.  ``depth`` is the range along the ray unless
        ``z_depth``.  Views of the renderer's buffers: the next call rewrites them."""
        h, w = image_shape_hw(image_shape)
        k = intrinsics_matrix(intrinsics)  # (both refusals come before anything touches the device)
        n = h * w
        self._ensure_buffers(n)
        self._extract_pose(pose)
        self.intrinsics_matrix.copy_(k.to(self.device))
        t, c = self.mapper.tsdf, self.config
        with torch.cuda.device(self.device):
            B.mapper_raycast(self._hit_points[:n], self._hit_normals[:n], self._hit_depths[:n], self._hit_mask[:n], self.intrinsics_matrix,
                             self.cam_position, self.cam_quaternion, t.block_data, t.block_visible, t.params, c.minimum_tsdf_weight,
                             c.depth_minimum_distance, c.depth_maximum_distance, (h, w), c.use_block_acceleration, z_depth)
        return self._hit_depths[:n].view(h, w), self._hit_normals[:n].view(h, w, 3), self._hit_mask[:n].view(h, w).bool()

    def render_color(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int]):
        """``(depth, normals, color uint8 [H, W, 3], valid)``; ``color`` is all zero: this mapper has no colour channel"""
        depth, normals, valid = self.render(intrinsics, pose, image_shape)
        h, w = depth.shape
        return depth, normals, self._hit_colors[: h * w].view(h, w, 3), valid

    def render_depth(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int], *, z_depth: bool = False) -> torch.Tensor:
        return self.render(intrinsics, pose, image_shape, z_depth=z_depth)[0]

    def render_normals(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int]) -> torch.Tensor:
        return self.render(intrinsics, pose, image_shape)[1]

    def render_color_only(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int]) -> torch.Tensor:
        return self.render_color(intrinsics, pose, image_shape)[2]

    def render_depth_colormap(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int]) -> torch.Tensor:
        depth, _, valid = self.render(intrinsics, pose, image_shape)
        return depth_to_colormap(depth, self.config.depth_minimum_distance, self.config.depth_maximum_distance, valid)

    def render_normal_colormap(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int]) -> torch.Tensor:
        _, normals, valid = self.render(intrinsics, pose, image_shape)
        return normals_to_colormap(normals, valid)

    def render_shaded(self, intrinsics: torch.Tensor, pose: Pose, image_shape: Tuple[int, int],
                      light_direction: Tuple[float, float, float] = (0.0, 0.0, 1.0), ambient: float = 0.3, use_color: bool = False) -> torch.Tensor:
        """Lambertian shading of a grey surface, uint8 [H, W, 3], black where nothing was hit; ``light_direction`` in the camera
        frame.  ``use_color`` defaults to False here (True in the reference): there is no colour channel to shade."""
        if use_color:
            raise NotImplementedError("render_shaded(use_color=True): this mapper has no colour channel")
        _, normals, valid = self.render(intrinsics, pose, image_shape)
        rotation = Pose(self.cam_position.view(1, 3), self.cam_quaternion.view(1, 4)).get_rotation_matrix()[0]
        light_world = rotation @ torch.tensor(light_direction, device=self.device, dtype=torch.float32)
        light_world = light_world / light_world.norm()
        shading = torch.clamp((normals * light_world.view(1, 1, 3)).sum(dim=-1), 0, 1)
        intensity = (ambient + (1.0 - ambient) * shading).unsqueeze(-1)
        shaded = torch.clamp(torch.ones_like(normals) * intensity * 255, 0, 255).to(torch.uint8)
        shaded[~valid] = 0
        return shaded


def image_shape_hw(image_shape) -> Tuple[int, int]:
    """``(H, W)`` as two positive ints, or ValueError"""
    try:
        h, w = (int(v) for v in image_shape)
    except (TypeError, ValueError):
        raise ValueError(f"image_shape must be (H, W), got {image_shape!r}") from None
    if h <= 0 or w <= 0:
        raise ValueError(f"image_shape must be (H, W) with both positive, got {image_shape!r}")
    return h, w


def intrinsics_matrix(intrinsics) -> torch.Tensor:
    """[3, 3] float32 from a [3, 3] matrix or from [fx, fy, cx, cy] (reference renderer.py:135-147)"""
    k = torch.as_tensor(intrinsics, dtype=torch.float32)
    if k.dim() == 2 and tuple(k.shape) == (3, 3):
        return k
    if k.dim() == 1 and k.numel() == 4:
        fx, fy, cx, cy = k.tolist()
        return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 0.0]], dtype=torch.float32)
    raise ValueError(f"intrinsics must be [3, 3] or [fx, fy, cx, cy], got shape {tuple(k.shape)}")


def depth_to_colormap(depth: torch.Tensor, depth_minimum_distance: float = 0.1, depth_maximum_distance: float = 5.0,
                      valid_mask: Optional[torch.Tensor] = None, invalid_color: Tuple[int, int, int] = (0, 0, 0)) -> torch.Tensor:
    """depth [H, W] metres -> uint8 [H, W, 3] by the reference's degree-5 fit of the turbo colormap over [minimum, maximum]
    (renderer.py:438-488); ``valid_mask`` defaults to ``depth > 0``, pixels outside it get ``invalid_color``"""
    if valid_mask is None:
        valid_mask = depth > 0
    t = torch.clamp((depth - depth_minimum_distance) / (depth_maximum_distance - depth_minimum_distance), 0, 1)
    r = torch.clamp(0.13572138 + t * (4.61539260 + t * (-42.66032258 + t * (132.13108234 + t * (-152.94239396 + t * 59.28637943)))), 0, 1)
    g = torch.clamp(0.09140261 + t * (2.19418839 + t * (4.84296658 + t * (-14.18503333 + t * (4.27729857 + t * 2.82956604)))), 0, 1)
    b = torch.clamp(0.10667330 + t * (12.64194608 + t * (-60.58204836 + t * (110.36276771 + t * (-89.90310912 + t * 27.34824973)))), 0, 1)
    color = (torch.stack([r, g, b], dim=-1) * 255).to(torch.uint8)
    color[~valid_mask] = torch.tensor(invalid_color, dtype=torch.uint8, device=depth.device)
    return color


def normals_to_colormap(normals: torch.Tensor, valid_mask: torch.Tensor) -> torch.Tensor:
    """normals [H, W, 3] -> uint8 [H, W, 3], x y z in [-1, 1] to r g b in [0, 255]; grey 128 outside ``valid_mask``
    (renderer.py:491-509)"""
    color = ((normals + 1.0) * 0.5 * 255).to(torch.uint8)
    color[~valid_mask] = 128
    return color
