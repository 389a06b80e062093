"""``Mapper``: depth frames -> dense TSDF -> exact fp16 ESDF, every per-voxel step on HIP (``csrc/mapper.hip``).

The reference's ``Mapper`` (``perception/mapper/mapper.py``) with the same calls: ``integrate(observation)`` fuses a
batch of depth images, ``compute_esdf()`` returns the ``VoxelGrid`` that ``SceneData.update_voxel_data`` puts in front of
the planners.  Where the reference keeps the blocks the camera has seen in a hash table over a pool, this mapper stores the
whole grid, padded to whole blocks, and keeps one byte per block, "ever visible", for "allocated".  Not built: decay and
block recycling, static obstacles, lidar, colour and feature channels, ``extract_mesh``, rendering, checkpoints,
``clear_blocks``, jump flooding, scatter seeding."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ...backends import mapper as B
from ...scene.types import VoxelGrid
from ...types import CameraObservation
from ...util.graph_capture import capture_graph
from .mapper_cfg import MapperCfg


@dataclass
class DenseTSDF:
    """the mapper's storage (``Mapper.tsdf``): the tensors themselves, not copies.  Block ``(bx, by, bz)`` of the padded grid
    is row ``(bz nby + by) nbx + bx``; voxel ``(lx, ly, lz)`` of a block is at ``lz BS^2 + ly BS + lx``."""

    #: fp16 [n_blocks, block_size^3, 2]: sum(sdf w), sum(w)
    block_data: torch.Tensor
    #: uint8, one byte per block (rounded up to a multiple of 4): the block was visible in some frame since the last reset
    block_visible: torch.Tensor
    #: uint8, likewise: the block was visible in the last frame
    frame_visible: torch.Tensor
    #: ``backends.mapper.MapperParams``: grid and block counts, origin, voxel size, truncation, depth range
    params: "B.MapperParams"

    @property
    def n_blocks(self) -> int:
        return self.params.n_blocks


class Mapper:
    """``Mapper(MapperCfg(...))``; ``integrate(obs)`` per frame, ``compute_esdf()`` when a planner needs the world.

    ``use_graph``: record the three ESDF stages into one hipGraph on the first ``compute_esdf`` and replay it afterwards
    (the origin and the voxel size are device tensors the recorded launches read)."""

    def __init__(self, config: MapperCfg, use_graph: bool = True):
        self.config = config
        self._device = torch.device(config.device)
        if config.dense_bytes > config.max_dense_bytes:  # (the configuration may have been edited after its own check)
            raise ValueError(f"the dense TSDF needs {config.dense_bytes} bytes, more than max_dense_bytes = {config.max_dense_bytes}")
        self._params = B.make_params(config.grid_shape, config.block_size, config.grid_center.tolist(), config.voxel_size,
                                     config.truncation_distance, config.depth_minimum_distance, config.depth_maximum_distance,
                                     config.minimum_tsdf_weight)
        dev, p = self._device, self._params
        self._tsdf = DenseTSDF(block_data=torch.zeros((p.n_blocks, p.block_voxels, 2), dtype=torch.float16, device=dev),
                               block_visible=torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=dev),
                               frame_visible=torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=dev), params=p)
        self._esdf_shape = tuple(int(v) for v in config.esdf_grid_shape)
        if max(self._esdf_shape) > B.ESDF_MAX_AXIS:
            raise ValueError(f"the ESDF grid {self._esdf_shape} has more than {B.ESDF_MAX_AXIS} cells along an axis")
        n = int(np.prod(self._esdf_shape))
        self._sites = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self._sites_scratch = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self._dist_field = torch.full(self._esdf_shape, 1e4, dtype=torch.float16, device=dev)
        self._esdf_origin = config.grid_center.to(device=dev, dtype=torch.float32).clone()
        self._esdf_voxel_size = torch.tensor([config.esdf_voxel_size], dtype=torch.float32, device=dev)
        self._last_esdf_origin = [float(v) for v in config.grid_center.tolist()]
        self._last_esdf_voxel_size = float(config.esdf_voxel_size)
        self._use_graph = bool(use_graph)
        self._graph = None
        self._frame_count = 0
        self._last_voxel_grid: Optional[VoxelGrid] = None

    # ------------------------------------------------------------------------------------------------ storage
    @property
    def tsdf(self) -> DenseTSDF:
        return self._tsdf

    @property
    def esdf_grid_shape(self):
        return self._esdf_shape

    # ------------------------------------------------------------------------------------------------ integration
    def integrate(self, *args, observation=None, camera_observation: Optional[CameraObservation] = None, lidar_observation=None) -> None:
        """fuse one batch of depth images: ``depth_image`` float32 metres ``(num_cameras, H, W)`` (``depth_to_meter`` is not
        applied), ``intrinsics`` ``(n, 3, 3)``, ``pose`` the cameras in the world (position, wxyz quaternion).  Positional
        ``integrate(obs)``, ``camera_observation=`` and the older ``observation=`` are accepted as in the reference."""
        if len(args) > 1:
            raise TypeError(f"integrate() takes at most one positional observation, got {len(args)}.")
        if args:
            if observation is not None or camera_observation is not None or lidar_observation is not None:
                raise TypeError("Positional observation cannot be combined with observation=, camera_observation=, or lidar_observation=.")
            observation = args[0]
        elif observation is not None and (camera_observation is not None or lidar_observation is not None):
            raise TypeError("observation= cannot be combined with camera_observation= or lidar_observation=.")
        if observation is not None:
            if isinstance(observation, CameraObservation):
                camera_observation = observation
            elif type(observation).__name__ == "LidarObservation":
                lidar_observation = observation
            else:
                raise TypeError(f"observation must be CameraObservation or LidarObservation, got {type(observation).__name__}.")
        if lidar_observation is not None:
            raise NotImplementedError("lidar_observation: lidar integration is not part of this mapper")
        if camera_observation is None:
            raise TypeError("integrate() requires a camera_observation or one positional observation.")
        depth, intrinsics, position, quaternion = self._camera_tensors(camera_observation)
        t = self._tsdf
        B.mapper_clear_mask(t.frame_visible)
        B.mapper_mark_blocks(t.frame_visible, t.block_visible, depth, intrinsics, position, quaternion, self._params)
        B.mapper_integrate(t.block_data, t.frame_visible, depth, intrinsics, position, quaternion, self._params)
        self._frame_count += 1
        self._last_voxel_grid = None

    def _camera_tensors(self, obs: CameraObservation):
        if obs.depth_image is None or obs.intrinsics is None or obs.pose is None:
            raise ValueError("integrate(): the observation needs depth_image, intrinsics and pose")
        f32 = dict(device=self._device, dtype=torch.float32)
        depth = obs.depth_image.to(**f32)
        depth = (depth.unsqueeze(0) if depth.dim() == 2 else depth).contiguous()
        cfg = self.config
        if depth.dim() != 3 or tuple(depth.shape[1:]) != (cfg.image_height, cfg.image_width) or depth.shape[0] > cfg.num_cameras:
            raise ValueError(f"integrate(): depth_image must be (n <= {cfg.num_cameras}, {cfg.image_height}, {cfg.image_width}), "
                             f"got {tuple(obs.depth_image.shape)}")
        n = int(depth.shape[0])
        intrinsics = obs.intrinsics.to(**f32).reshape(-1, 3, 3)
        position = obs.pose.position.to(**f32).reshape(-1, 3)
        quaternion = obs.pose.quaternion.to(**f32).reshape(-1, 4)
        for name, t in (("intrinsics", intrinsics), ("pose", position), ("pose", quaternion)):
            if t.shape[0] != n:
                raise ValueError(f"integrate(): {name} holds {t.shape[0]} cameras, depth_image {n}")
        return depth, intrinsics.contiguous(), position.contiguous(), quaternion.contiguous()

    # ------------------------------------------------------------------------------------------------ ESDF
    def _esdf_chain(self) -> None:
        """seed, the three passes of the nearest-site transform, signed distance: five launches of fixed dimensions"""
        t = self._tsdf
        B.mapper_esdf_seed(self._sites, t.block_data, t.block_visible, self._esdf_origin, self._esdf_voxel_size, self._params, self._esdf_shape)
        nearest = B.mapper_edt(self._sites, self._sites_scratch, self._esdf_shape)
        B.mapper_esdf_distance(self._dist_field, nearest, t.block_data, t.block_visible, self._esdf_origin, self._esdf_voxel_size,
                               self._params, self._esdf_shape)

    def compute_esdf(self, esdf_origin: Optional[torch.Tensor] = None, esdf_voxel_size: Optional[float] = None) -> VoxelGrid:
        """the ESDF of the current TSDF as a ``VoxelGrid`` named ``"block_sparse_esdf_grid"`` (negative inside, 1e4 where no
        surface has been seen at all); its ``feature_tensor`` is the mapper's own fp16 buffer, rewritten by the next call.
        ``esdf_origin`` / ``esdf_voxel_size`` move / rescale the grid (a sliding window) and stay in force afterwards."""
        if esdf_origin is not None:
            origin = torch.as_tensor(esdf_origin, dtype=torch.float32).reshape(3)
            self._esdf_origin.copy_(origin)
            self._last_esdf_origin = [float(v) for v in origin.tolist()]
        if esdf_voxel_size is not None:
            if not float(esdf_voxel_size) > 0.0:
                raise ValueError(f"esdf_voxel_size must be positive: {esdf_voxel_size}")
            self._esdf_voxel_size.fill_(float(esdf_voxel_size))
            self._last_esdf_voxel_size = float(esdf_voxel_size)
        with torch.cuda.device(self._device):
            if not self._use_graph:
                self._esdf_chain()
            else:
                if self._graph is None:
                    self._graph, _ = capture_graph(self._esdf_chain, device=self._device)
                self._graph.replay()
        self._last_voxel_grid = self.get_voxel_grid()
        return self._last_voxel_grid

    def get_voxel_grid(self) -> VoxelGrid:
        """(reference ``integrator_esdf.py`` get_voxel_grid: pose = the last origin and no rotation, dims = shape x voxel size)"""
        vs = self._last_esdf_voxel_size
        return VoxelGrid(name="block_sparse_esdf_grid", pose=[*self._last_esdf_origin, 1.0, 0.0, 0.0, 0.0],
                         dims=[n * vs for n in self._esdf_shape], voxel_size=vs, feature_tensor=self._dist_field)

    # ------------------------------------------------------------------------------------------------ editing
    def reset(self) -> None:
        """an empty map: nothing observed, no block ever visible"""
        t = self._tsdf
        t.block_data.zero_()
        t.block_visible.zero_()
        t.frame_visible.zero_()
        self._frame_count = 0
        self._last_voxel_grid = None

    def _blocks_view(self, flat: torch.Tensor) -> torch.Tensor:
        p = self._params
        return flat[: p.n_blocks].view(p.nbz, p.nby, p.nbx, *flat.shape[1:])

    def clear_region(self, bounds_min, bounds_max) -> int:
        """zero every voxel of every block the world-space box touches (the blocks stay "ever visible"); returns how many of
        them were ever visible.  The cached grid is dropped: call ``compute_esdf`` again."""
        p = self._params
        lo_w = np.minimum(np.asarray(bounds_min, np.float64).reshape(3), np.asarray(bounds_max, np.float64).reshape(3))
        hi_w = np.maximum(np.asarray(bounds_min, np.float64).reshape(3), np.asarray(bounds_max, np.float64).reshape(3))
        grid = np.array([p.grid_w, p.grid_h, p.grid_d], np.float64)
        origin = np.array(list(p.origin), np.float64)
        lo = np.floor(((lo_w - origin) / float(p.voxel_size) + 0.5 * grid) / int(p.block_size)).astype(np.int64)
        hi = np.floor(((hi_w - origin) / float(p.voxel_size) + 0.5 * grid) / int(p.block_size)).astype(np.int64)
        nb = np.array([p.nbx, p.nby, p.nbz], np.int64)
        lo, hi = np.maximum(lo, 0), np.minimum(hi, nb - 1)
        if (lo > hi).any():
            return 0
        sel = (slice(int(lo[2]), int(hi[2]) + 1), slice(int(lo[1]), int(hi[1]) + 1), slice(int(lo[0]), int(hi[0]) + 1))
        n_clear = int(self._blocks_view(self._tsdf.block_visible)[sel].sum().item())
        self._blocks_view(self._tsdf.block_data)[sel] = 0
        if n_clear > 0:
            self._last_voxel_grid = None
        return n_clear

    # ------------------------------------------------------------------------------------------------ read-outs
    def extract_occupied_voxels(self, surface_only: bool = False, sdf_threshold: Optional[float] = None) -> torch.Tensor:
        """centres ``[m, 3]`` of the observed voxels of ever-visible blocks with ``sdf <= 0``, or with ``|sdf| < sdf_threshold``
        (default: the voxel size) when ``surface_only``; as the reference's rule, a block's padding voxels count like any other"""
        p, t = self._params, self._tsdf
        threshold = float(self.config.voxel_size if sdf_threshold is None else sdf_threshold)
        flags = torch.empty((p.n_blocks, p.block_voxels), dtype=torch.uint8, device=self._device)
        with torch.cuda.device(self._device):
            B.mapper_occupied_flags(flags, t.block_data, t.block_visible, p, surface_only, threshold)
        block, local = torch.nonzero(flags, as_tuple=True)
        bs = int(p.block_size)
        g = torch.stack([(block % p.nbx) * bs + local % bs, ((block // p.nbx) % p.nby) * bs + (local // bs) % bs,
                         (block // (p.nbx * p.nby)) * bs + local // (bs * bs)], dim=1).to(torch.float32)
        half = torch.tensor([p.grid_w, p.grid_h, p.grid_d], dtype=torch.float32, device=self._device) * 0.5
        origin = torch.tensor(list(p.origin), dtype=torch.float32, device=self._device)
        return origin + (g + 0.5 - half) * float(p.voxel_size)

    def memory_usage_mb(self) -> float:
        t = self._tsdf
        tensors = (t.block_data, t.block_visible, t.frame_visible, self._sites, self._sites_scratch, self._dist_field)
        return sum(x.numel() * x.element_size() for x in tensors) / (1024.0 * 1024.0)

    def get_stats(self) -> dict:
        """``frame_count``, ``total_blocks``, ``visible_blocks`` (ever), ``last_frame_blocks``, ``block_size``, ``tsdf_grid_shape``
        (nz, ny, nx), ``esdf_grid_shape`` (nx, ny, nz), ``memory_mb``"""
        p, t = self._params, self._tsdf
        return {"frame_count": self._frame_count, "total_blocks": p.n_blocks,
                "visible_blocks": int(t.block_visible[: p.n_blocks].sum().item()),
                "last_frame_blocks": int(t.frame_visible[: p.n_blocks].sum().item()), "block_size": int(p.block_size),
                "tsdf_grid_shape": tuple(self.config.grid_shape), "esdf_grid_shape": self._esdf_shape, "memory_mb": self.memory_usage_mb()}
