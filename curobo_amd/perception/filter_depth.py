"""Depth image filtering (reference ``curobo/_src/perception/filter_depth.py``): range check, flying-pixel rejection and
bilateral smoothing of batched ``(B, H, W)`` depth images in one HIP launch (three for kernel sizes >= 7), into
pre-allocated buffers.  A single image is passed as ``depth.unsqueeze(0)``."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..backends import perception as _backend


@dataclass
class FilterDepthConfig:
    """``flying_pixel_threshold``: 0 (permissive) .. 1 (aggressive), ``None`` switches the test off;
    ``bilateral_kernel_size``: odd, ``None`` switches smoothing off; sigmas in pixels / metres."""

    depth_minimum_distance: float = 0.1
    depth_maximum_distance: float = 10.0
    flying_pixel_threshold: Optional[float] = 0.5
    bilateral_kernel_size: Optional[int] = 5
    bilateral_sigma_spatial: float = 2.0
    bilateral_sigma_depth: float = 0.05


class FilterDepth:
    def __init__(self, image_shape: Tuple[int, int], depth_minimum_distance: float = 0.1, depth_maximum_distance: float = 10.0,
                 flying_pixel_threshold: Optional[float] = 0.5, bilateral_kernel_size: Optional[int] = 5,
                 bilateral_sigma_spatial: float = 10.0, bilateral_sigma_depth: float = 0.1, device: str = "cuda", num_batch: int = 1):
        self.device = torch.device(device)
        self.image_shape = image_shape
        self.num_batch = max(int(num_batch), 1)
        H, W = image_shape
        B = self.num_batch
        self.config = FilterDepthConfig(
            depth_minimum_distance=depth_minimum_distance, depth_maximum_distance=depth_maximum_distance,
            flying_pixel_threshold=flying_pixel_threshold, bilateral_kernel_size=bilateral_kernel_size,
            bilateral_sigma_spatial=bilateral_sigma_spatial, bilateral_sigma_depth=bilateral_sigma_depth)
        if bilateral_kernel_size is not None and bilateral_kernel_size % 2 == 0:
            raise ValueError(f"bilateral_kernel_size must be odd, got {bilateral_kernel_size}")
        self._setup_kernel_params()
        self._depth_out = torch.zeros((B, H, W), dtype=torch.float32, device=self.device)
        self._valid_mask_out = torch.zeros((B, H, W), dtype=torch.uint8, device=self.device)
        # kernel sizes from 7 on run as three passes (range + flying pixels, horizontal, vertical) through two scratch images
        self._use_separable = bilateral_kernel_size is not None and bilateral_kernel_size >= 7
        self._depth_temp = torch.zeros((B, H, W), dtype=torch.float32, device=self.device) if self._use_separable else None
        self._depth_temp2 = torch.zeros((B, H, W), dtype=torch.float32, device=self.device) if self._use_separable else None

    def _setup_kernel_params(self) -> None:
        cfg = self.config
        if cfg.flying_pixel_threshold is not None:
            max_tol, min_tol = 0.08, 0.005  # threshold 0 -> 8 % of the depth, 0.5 -> 2 %, 1 -> 0.5 %
            self._flying_tolerance = max_tol * (min_tol / max_tol) ** cfg.flying_pixel_threshold
            self._enable_flying = 1
        else:
            self._flying_tolerance, self._enable_flying = 0.0, 0
        if cfg.bilateral_kernel_size is not None:
            self._bilateral_radius = cfg.bilateral_kernel_size // 2
            self._sigma_spatial_sq2 = 2.0 * cfg.bilateral_sigma_spatial ** 2
            self._sigma_depth_sq2 = 2.0 * cfg.bilateral_sigma_depth ** 2
            self._enable_bilateral = 1
        else:
            self._bilateral_radius, self._sigma_spatial_sq2, self._sigma_depth_sq2, self._enable_bilateral = 0, 1.0, 1.0, 0

    def __call__(self, depth_image: torch.Tensor, depth_out: Optional[torch.Tensor] = None,
                 valid_mask_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(B, H, W) float32 depth -> (filtered depth with rejected pixels 0, bool mask of the pixels kept)"""
        if depth_image.dim() != 3:
            raise ValueError("FilterDepth expects a batched depth tensor of shape "
                             f"(B, H, W); got {tuple(depth_image.shape)}. For a single "
                             "image, pass depth.unsqueeze(0).")
        B, H, W = depth_image.shape
        out_depth, out_mask = self._acquire_buffers(B, H, W, depth_out, valid_mask_out)
        temp_a = temp_b = None
        if self._use_separable and self._enable_bilateral:
            if self._shape_match(B, H, W) and self._depth_temp is not None:
                temp_a, temp_b = self._depth_temp, self._depth_temp2
            else:
                temp_a = torch.zeros((B, H, W), dtype=torch.float32, device=self.device)
                temp_b = torch.zeros((B, H, W), dtype=torch.float32, device=self.device)
        cfg = self.config
        _backend.filter_depth(out_depth, out_mask, depth_image, temp_a, temp_b, cfg.depth_minimum_distance,
                              cfg.depth_maximum_distance, bool(self._enable_flying), self._flying_tolerance,
                              cfg.bilateral_kernel_size if self._enable_bilateral else 0, self._sigma_spatial_sq2,
                              self._sigma_depth_sq2)
        return out_depth, out_mask.bool()

    def _shape_match(self, B: int, H: int, W: int) -> bool:
        return H == self.image_shape[0] and W == self.image_shape[1] and B == self.num_batch

    def _acquire_buffers(self, B: int, H: int, W: int, depth_out: Optional[torch.Tensor],
                         valid_mask_out: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """the caller's buffers when given, else the pre-allocated ones when the shape is the one of the constructor, else new ones"""
        for buf, name in ((depth_out, "depth_out"), (valid_mask_out, "valid_mask_out")):
            if buf is not None and tuple(buf.shape) != (B, H, W):
                raise ValueError(f"{name} must have shape (B, H, W)=({B}, {H}, {W}); got {tuple(buf.shape)}")
        match = self._shape_match(B, H, W)
        if depth_out is None:
            depth_out = self._depth_out if match else torch.zeros((B, H, W), dtype=torch.float32, device=self.device)
        if valid_mask_out is None:
            valid_mask_out = self._valid_mask_out if match else torch.zeros((B, H, W), dtype=torch.uint8, device=self.device)
        return depth_out, valid_mask_out

    def update_config(self, depth_minimum_distance: Optional[float] = None, depth_maximum_distance: Optional[float] = None,
                      flying_pixel_threshold: Optional[float] = None, bilateral_sigma_depth: Optional[float] = None) -> None:
        """change parameters without touching the buffers; ``None`` keeps a value, ``flying_pixel_threshold=0`` switches the test off"""
        if depth_minimum_distance is not None:
            self.config.depth_minimum_distance = depth_minimum_distance
        if depth_maximum_distance is not None:
            self.config.depth_maximum_distance = depth_maximum_distance
        if flying_pixel_threshold is not None:
            self.config.flying_pixel_threshold = None if flying_pixel_threshold == 0 else flying_pixel_threshold
        if bilateral_sigma_depth is not None:
            self.config.bilateral_sigma_depth = bilateral_sigma_depth
        self._setup_kernel_params()

    @classmethod
    def from_config(cls, config: FilterDepthConfig, image_shape: Tuple[int, int], device: str = "cuda", num_batch: int = 1) -> "FilterDepth":
        return cls(image_shape=image_shape, depth_minimum_distance=config.depth_minimum_distance,
                   depth_maximum_distance=config.depth_maximum_distance, flying_pixel_threshold=config.flying_pixel_threshold,
                   bilateral_kernel_size=config.bilateral_kernel_size, bilateral_sigma_spatial=config.bilateral_sigma_spatial,
                   bilateral_sigma_depth=config.bilateral_sigma_depth, device=device, num_batch=num_batch)
