"""``Mapper``: depth frames -> dense TSDF -> exact fp16 ESDF, every per-voxel step on HIP (``csrc/mapper.hip``).

The reference's ``Mapper`` (``perception/mapper/mapper.py``) with the same calls: ``integrate(observation)`` fuses a
batch of depth images, ``compute_esdf()`` returns the ``VoxelGrid`` that ``SceneData.update_voxel_data`` puts in front of
the planners.  Where the reference keeps the blocks the camera has seen in a hash table over a pool, this mapper stores the
whole grid, padded to whole blocks, and keeps one byte per block, "ever visible", for "allocated".  ``extract_mesh()`` is the
reference's third read-out: marching cubes over the ever-visible blocks, as a ``Mesh``.  ``render*()`` ray-cast the TSDF into
depth, normal and shaded images (``renderer.py``); ``pose_refiner.py`` aligns a new depth image to the map before it is
integrated.  The map forgets when asked to: per-frame weight decay (``time_decay`` / ``frustum_decay``, the constructor's
arguments) and the recycling of blocks whose weight has decayed to nothing (``decay.py``).  Lidar range images
(``LidarObservation``) are fused into the same voxels by two launches of their own (``csrc/mapper_lidar.hip``), alone or in one
frame with the cameras; the sensors are described by the constructor's ``lidar=MapperLidarCfg(...)``.  Not built: static
obstacles, colour and feature channels (rendered colour is zero; a lidar's ``rgb_image`` is checked and not used), checkpoints,
``clear_blocks``, jump flooding, scatter seeding."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ...backends import mapper as B
from ...scene.types import Mesh, VoxelGrid
from ...types import CameraObservation, LidarObservation
from ...util.graph_capture import capture_graph
from . import decay as D
from . import mc_table
from .mapper_cfg import MapperCfg, MapperLidarCfg


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
    #: uint8, likewise: the block was visible to a LIDAR in the last frame that carried lidars -- what the lidar integration reads,
    #: a subset of ``frame_visible`` in that frame (made here when not given)
    lidar_frame_visible: Optional[torch.Tensor] = None
    #: uint8, likewise: the block was recycled by the last decay launch (made here when not given)
    block_recycled: Optional[torch.Tensor] = None

    def __post_init__(self):
        if self.lidar_frame_visible is None:
            self.lidar_frame_visible = torch.zeros_like(self.block_visible)
        if self.block_recycled is None:
            self.block_recycled = torch.zeros_like(self.block_visible)

    @property
    def n_blocks(self) -> int:
        return self.params.n_blocks


class _LidarAtConstruction(type):
    """``Mapper(cfg, ..., lidar=MapperLidarCfg(...))``: the keyword is taken here and handed to ``Mapper.configure_lidar``, because
    tests/test_mapper_decay_host.py pins the parameter list of ``Mapper.__init__`` as it was and existing tests stay as they are.
    Once that pin is lifted ``lidar`` becomes a parameter of ``__init__`` like any other and this class goes."""

    def __call__(cls, *args, lidar: Optional[MapperLidarCfg] = None, **kwargs):
        mapper = super().__call__(*args, **kwargs)
        mapper.configure_lidar(lidar)
        return mapper


class Mapper(metaclass=_LidarAtConstruction):
    """``Mapper(MapperCfg(...))``; ``integrate(obs)`` per frame, ``compute_esdf()`` when a planner needs the world.

    ``lidar=MapperLidarCfg(num_sensors=..., image_height=..., image_width=...)``: the lidars whose ``LidarObservation`` this mapper
    integrates, alone or together with a ``CameraObservation`` in one frame; without it a ``lidar_observation`` is refused.  The
    setting is the constructor's and not ``MapperCfg``'s, whose ``lidar_num_sensors`` > 0 still refuses: tests/test_mapper_host.py
    pins that refusal; lifting it is a follow-up (build the ``MapperLidarCfg`` from ``MapperCfg.lidar_*`` and hand it on).

    ``use_graph``: record the three ESDF stages into one hipGraph on the first ``compute_esdf`` and replay it afterwards
    (the origin and the voxel size are device tensors the recorded launches read).

    ``time_decay`` / ``frustum_decay`` in (0, 1], the reference's ``BlockSparseTSDFIntegratorCfg`` fields: with either below 1
    every ``integrate`` but the first after construction or ``reset()`` begins with the frame decay (reference
    ``integrator_tsdf.py:611-675``): every ever-visible block's weights times ``time_decay``, those in the union of the frusta of
    the observation's cameras times ``time_decay frustum_decay``, and blocks whose weight has gone recycled.  With both at 1
    nothing is launched.  They are set here, not in ``MapperCfg``, whose ``decay_factor`` / ``frustum_decay_factor`` still refuse
    values other than 1: tests/test_mapper_host.py pins that refusal; lifting it is two lines in ``MapperCfg.__post_init__``
    and passing the two fields on to this constructor."""

    def __init__(self, config: MapperCfg, use_graph: bool = True, time_decay: float = 1.0, frustum_decay: float = 1.0):
        self.config = config
        self._time_decay = D.check_factor("time_decay", time_decay)
        self._frustum_decay = D.check_factor("frustum_decay", frustum_decay)
        self._device = torch.device(config.device)
        if config.dense_bytes > config.max_dense_bytes:  # (the configuration may have been edited after its own check)
            raise ValueError(f"the dense TSDF needs {config.dense_bytes} bytes, more than max_dense_bytes = {config.max_dense_bytes}")
        self._params = B.make_params(config.grid_shape, config.block_size, config.grid_center.tolist(), config.voxel_size,
                                     config.truncation_distance, config.depth_minimum_distance, config.depth_maximum_distance,
                                     config.minimum_tsdf_weight)
        dev, p = self._device, self._params
        self._tsdf = DenseTSDF(block_data=torch.zeros((p.n_blocks, p.block_voxels, 2), dtype=torch.float16, device=dev),
                               block_visible=torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=dev),
                               frame_visible=torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=dev), params=p,
                               block_recycled=torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=dev))
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
        self._mc_tables = None  # (case table, edge owners) on the device, from the first extract_mesh on
        self._renderer = None   # from the first render on
        self._lidar: Optional[MapperLidarCfg] = None

    def configure_lidar(self, lidar: Optional[MapperLidarCfg]) -> None:
        """what the constructor's ``lidar=`` does: the lidars of the ``LidarObservation`` frames to come (``None``: none, refuse them)"""
        if lidar is not None and not isinstance(lidar, MapperLidarCfg):
            raise TypeError(f"lidar must be a MapperLidarCfg, got {type(lidar).__name__}")
        limit = None if lidar is None else lidar.max_visible_blocks_per_lidar_integration
        if limit is not None and limit > self._params.n_blocks:  # (the reference's bound, mapper_cfg.py:290-300; no effect otherwise)
            raise ValueError(f"max_visible_blocks_per_lidar_integration must satisfy 0 < value <= {self._params.n_blocks}, got {limit}")
        self._lidar = lidar

    @property
    def lidar_config(self) -> Optional[MapperLidarCfg]:
        return self._lidar

    # ------------------------------------------------------------------------------------------------ storage
    @property
    def tsdf(self) -> DenseTSDF:
        return self._tsdf

    @property
    def esdf_grid_shape(self):
        return self._esdf_shape

    # ------------------------------------------------------------------------------------------------ integration
    def integrate(self, *args, observation=None, camera_observation: Optional[CameraObservation] = None,
                  lidar_observation: Optional[LidarObservation] = None) -> None:
        """fuse one frame.  A ``CameraObservation``: a batch of depth images, ``depth_image`` float32 metres ``(num_cameras, H, W)``
        (``depth_to_meter`` is not applied), ``intrinsics`` ``(n, 3, 3)``, ``pose`` the cameras in the world (position, wxyz
        quaternion).  A ``LidarObservation`` (with ``lidar=`` given to the constructor): ``range_image`` float32 metres
        ``(num_sensors, H, W)``, ``pose``, ``valid_range_m`` and ``elevation_range_rad`` ``(n, 2)``.  Positional ``integrate(obs)``,
        ``camera_observation=``, ``lidar_observation=`` and the older ``observation=`` are accepted as in the reference; one call may
        carry a camera and a lidar observation, which make ONE frame (reference ``integrator_tsdf.py:451-493``): the frame decay once
        over the union of both kinds of frusta, the camera stages, then the lidar stages."""
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
            elif isinstance(observation, LidarObservation):
                lidar_observation = observation
            else:
                raise TypeError(f"observation must be CameraObservation or LidarObservation, got {type(observation).__name__}.")
        if lidar_observation is not None and self._lidar is None:
            raise NotImplementedError("lidar_observation: this mapper was built without lidars; enable lidar integration with "
                                      "Mapper(cfg, lidar=MapperLidarCfg(num_sensors=..., image_height=..., image_width=...))")
        if camera_observation is None and lidar_observation is None:
            raise TypeError("integrate() requires a camera_observation, a lidar_observation or one positional observation.")
        camera = None if camera_observation is None else self._camera_tensors(camera_observation)
        lidar = None if lidar_observation is None else self._lidar_tensors(lidar_observation)
        t = self._tsdf
        if self._frame_count > 0 and (self._time_decay < 1.0 or self._frustum_decay < 1.0):  # integrator_tsdf.py:617-620
            if lidar is None:
                depth, intrinsics, position, quaternion = camera
                D.decay_frustum_aware_multi_camera(t, intrinsics, position, quaternion, depth.shape[1:], self.config.depth_minimum_distance,
                                                   self.config.depth_maximum_distance, self._time_decay, self._frustum_decay)
            else:
                kw = {}
                if camera is not None:
                    kw = dict(camera_intrinsics=camera[1], camera_positions=camera[2], camera_quaternions=camera[3],
                              camera_img_shape=tuple(camera[0].shape[1:]))
                D.decay_frustum_aware_multi_sensor(t, **kw, camera_depth_minimum_distance=self.config.depth_minimum_distance,
                                                   camera_depth_maximum_distance=self.config.depth_maximum_distance, lidar_positions=lidar[1],
                                                   lidar_quaternions=lidar[2], lidar_valid_range_m=lidar[3], lidar_elevation_range_rad=lidar[4],
                                                   lidar_img_shape=tuple(lidar[0].shape[1:]), time_decay=self._time_decay,
                                                   frustum_decay=self._frustum_decay)
        B.mapper_clear_mask(t.frame_visible)
        if camera is not None:
            B.mapper_mark_blocks(t.frame_visible, t.block_visible, *camera, self._params)
            B.mapper_integrate(t.block_data, t.frame_visible, *camera, self._params)
        if lidar is not None:  # after the cameras (integrator_tsdf.py:485-492); the lidar sums go to the blocks the LIDARS marked
            vs = float(self.config.voxel_size)
            B.mapper_clear_mask(t.lidar_frame_visible)
            B.mapper_lidar_mark_blocks(t.lidar_frame_visible, t.frame_visible, t.block_visible, *lidar, self._params)
            B.mapper_lidar_integrate(t.block_data, t.lidar_frame_visible, *lidar, self._params,
                                     float(self._lidar.linear_interpolation_max_allowable_difference_vox) * vs,
                                     float(self._lidar.nearest_interpolation_max_allowable_dist_to_ray_vox) * vs)
        self._frame_count += 1
        self._last_voxel_grid = None

    def _lidar_tensors(self, obs: LidarObservation):
        """the observation checked by the reference's rules (integrator_tsdf.py:709-835; there the colour image is required, here it
        may be left out, and it is not used): (range_image, position, quaternion, valid_range_m, elevation_range_rad) on the device"""
        cfg = self._lidar
        expected = (cfg.num_sensors, cfg.image_height, cfg.image_width)
        r = obs.range_image
        if r is None:
            raise ValueError("LidarObservation.range_image is required.")
        if r.dim() != 3:
            raise ValueError(f"range_image must be (num_lidars, H, W), got shape {tuple(r.shape)}.")
        if tuple(r.shape) != expected:
            raise ValueError(f"range_image shape mismatch: expected {expected}, got {tuple(r.shape)}.")
        if r.dtype != torch.float32:
            raise ValueError(f"range_image dtype must be torch.float32, got {r.dtype}.")
        if obs.rgb_image is not None:
            if tuple(obs.rgb_image.shape) != expected + (3,):
                raise ValueError(f"rgb_image shape mismatch: expected {expected + (3,)}, got {tuple(obs.rgb_image.shape)}.")
            if obs.rgb_image.dtype != torch.uint8:
                raise ValueError(f"rgb_image dtype must be torch.uint8, got {obs.rgb_image.dtype}.")
        if obs.feature_grid is not None:
            raise NotImplementedError("LidarObservation.feature_grid was provided but feature_dim == 0: feature channels are not part of "
                                      "this mapper")
        if obs.pose is None:
            raise ValueError("LidarObservation.pose is required.")
        n = cfg.num_sensors
        f32 = dict(device=self._device, dtype=torch.float32)
        position, quaternion = obs.pose.position.to(**f32).reshape(-1, 3), obs.pose.quaternion.to(**f32).reshape(-1, 4)
        if position.shape[0] != n or quaternion.shape[0] != n:
            raise ValueError(f"LidarObservation.pose holds {position.shape[0]} lidars, range_image {n}")
        bounds = []
        for name in ("valid_range_m", "elevation_range_rad"):
            v = getattr(obs, name)
            if v is None:
                raise ValueError(f"LidarObservation.{name} is required.")
            if tuple(v.shape) != (n, 2):
                raise ValueError(f"{name} must be (num_lidars, 2), got shape {tuple(v.shape)}.")
            if v.dtype != torch.float32:
                raise ValueError(f"{name} dtype must be torch.float32, got {v.dtype}.")
            bounds.append(v.to(**f32).contiguous())
        if cfg.image_height == 1 and not torch.allclose(bounds[1][:, 0], bounds[1][:, 1]):
            raise ValueError("Planar LiDAR with image_height == 1 requires elevation_range_rad[:, 0] == elevation_range_rad[:, 1].")
        return r.to(**f32).contiguous(), position.contiguous(), quaternion.contiguous(), bounds[0], bounds[1]

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
        t.lidar_frame_visible.zero_()
        t.block_recycled.zero_()
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

    def decay_and_recycle(self, decay_factor: float = 0.95) -> int:
        """every weight times ``decay_factor`` in (0, 1], then the blocks whose weights sum to less than ``0.01 block_size^3 / 8^3``
        recycled: no longer visible, their voxels zero.  Returns how many were (one read back to the host).  The cached grid is
        dropped: call ``compute_esdf`` again."""
        n = D.decay_and_recycle(self._tsdf, D.check_factor("decay_factor", decay_factor))
        self._last_voxel_grid = None
        return n

    def recycle_empty_blocks(self) -> int:
        """``decay_and_recycle`` without the decay (reference ``integrator_tsdf.py:837-846``)"""
        return self.decay_and_recycle(1.0)

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

    def extract_mesh(self, refine_iterations: int = 2, surface_only: bool = True, level: float = 0.0) -> Mesh:
        """the iso-surface ``sdf = level`` of the TSDF as a ``Mesh`` named ``"block_sparse_tsdf_mesh"`` in the world frame, its
        ``vertices``, ``faces``, ``vertex_normals`` and ``vertex_colors`` the device tensors of ``extract_mesh_tensors``"""
        vertices, triangles, normals, colors = self.extract_mesh_tensors(level=level, surface_only=surface_only, refine_iterations=refine_iterations)
        return Mesh(name="block_sparse_tsdf_mesh", pose=[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], vertices=vertices, faces=triangles,
                    vertex_normals=normals, vertex_colors=colors)

    def extract_mesh_tensors(self, level: float = 0.0, surface_only: bool = False, refine_iterations: int = 0):
        """marching cubes over the ever-visible blocks (``csrc/mapper.hip``, the ``mapper_mesh_*`` launches): ``(vertices`` float32
        [V, 3], ``triangles`` int32 [T, 3], ``normals`` float32 [V, 3], ``colors`` uint8 [V, 3]) on the mapper's device; four
        ``(0, 3)`` tensors for an empty map or one without a surface.  ``colors`` is all zero: this mapper has no colour channel.

        A cube's corners are eight voxel centres; it is meshed when all eight are observed (weight >= ``minimum_tsdf_weight``, in
        ever-visible blocks) and their values ``sdf - level`` change sign -- with ``surface_only`` also some ``|sdf - level|`` is below
        the truncation distance, which leaves out the sign change between free space and the clamped far side of a surface.
        ``refine_iterations`` Newton steps along the trilinear gradient follow the linear interpolation; the normals are central
        differences of the nearest voxels.  ``(v1 - v0) x (v2 - v0)`` of a triangle points to the positive (free) side.  Triangles
        at the rim of the observed region whose neighbour cube is not meshed are dropped, and so are triangles without area, as in
        the reference.  The order of both lists is (block, voxel, axis or table order) and the same from run to run.

        The sizes depend on the data, so nothing here is captured into a graph: four launches on the current stream, and THREE
        reads of totals back to the host (the visible blocks; vertices and table triangles; triangles kept)."""
        p, t, dev = self._params, self._tsdf, self._device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        empty = (torch.zeros((0, 3), **f32), torch.zeros((0, 3), **i32), torch.zeros((0, 3), **f32), torch.zeros((0, 3), dtype=torch.uint8, device=dev))
        with torch.cuda.device(dev):
            visible = t.block_visible[: p.n_blocks] != 0
            block_list = torch.nonzero(visible).reshape(-1).to(torch.int32)  # read 1: how many blocks (ascending rows)
            n_slots = int(block_list.numel())
            if n_slots == 0:
                return empty
            if self._mc_tables is None:
                self._mc_tables = (torch.as_tensor(mc_table.triangle_table(), device=dev).contiguous(),
                                   torch.as_tensor(mc_table.EDGE_OWNER.astype(np.int8), device=dev).contiguous())
            table, edge_owner = self._mc_tables
            n_voxels = n_slots * p.block_voxels
            cube_case, vert_count, tri_count = (torch.empty(n_voxels, dtype=torch.uint8, device=dev) for _ in range(3))
            B.mapper_mesh_classify(cube_case, vert_count, tri_count, t.block_data, t.block_visible, block_list, table, p, level, surface_only)
            vert_end, tri_end = torch.cumsum(vert_count, 0, dtype=torch.int32), torch.cumsum(tri_count, 0, dtype=torch.int32)
            n_vertices, n_raw = (int(v) for v in torch.stack([vert_end[-1], tri_end[-1]]).tolist())  # read 2
            if n_vertices == 0 or n_raw == 0:
                return empty
            vertices, normals = torch.empty((n_vertices, 3), **f32), torch.empty((n_vertices, 3), **f32)
            vert_ids = torch.empty((n_voxels, 3), **i32)
            B.mapper_mesh_vertices(vertices, normals, vert_ids, vert_count, vert_end - vert_count, t.block_data, t.block_visible, block_list, p,
                                   level, refine_iterations)
            block_slot = torch.where(visible, torch.cumsum(visible, 0, dtype=torch.int32) - 1, -1).to(torch.int32).contiguous()
            raw, keep = torch.empty((n_raw, 3), **i32), torch.empty(n_raw, dtype=torch.uint8, device=dev)
            B.mapper_mesh_triangles(raw, keep, cube_case, tri_count, tri_end - tri_count, vert_ids, vertices, block_list, block_slot, table,
                                    edge_owner, p)
            keep_end = torch.cumsum(keep, 0, dtype=torch.int32)
            n_triangles = int(keep_end[-1].item())  # read 3
            if n_triangles == 0:
                return empty
            triangles = torch.empty((n_triangles, 3), **i32)
            B.mapper_mesh_compact(triangles, raw, keep, keep_end - keep)
        return vertices, triangles, normals, torch.zeros((n_vertices, 3), dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------------------------------------ rendering
    def _get_renderer(self):
        """the mapper's ``BlockSparseTSDFRenderer``, made on first use (reference mapper.py:504-512)"""
        if self._renderer is None:
            from .renderer import BlockSparseTSDFRenderer

            self._renderer = BlockSparseTSDFRenderer(self)
        return self._renderer

    def render(self, intrinsics: torch.Tensor, pose, image_shape, **kwargs):
        """``(depth [H, W], normals [H, W, 3], valid [H, W] bool)`` of the TSDF seen from ``pose``: ``renderer.py``, whose notes on the
        depth's meaning (range along the ray unless ``z_depth=True``) and on the returned views apply"""
        return self._get_renderer().render(intrinsics, pose, image_shape, **kwargs)

    def render_color(self, intrinsics: torch.Tensor, pose, image_shape):
        return self._get_renderer().render_color(intrinsics, pose, image_shape)

    def render_depth(self, intrinsics: torch.Tensor, pose, image_shape, **kwargs) -> torch.Tensor:
        return self._get_renderer().render_depth(intrinsics, pose, image_shape, **kwargs)

    def render_color_only(self, intrinsics: torch.Tensor, pose, image_shape) -> torch.Tensor:
        return self._get_renderer().render_color_only(intrinsics, pose, image_shape)

    def render_shaded(self, intrinsics: torch.Tensor, pose, image_shape, light_direction=(0.0, 0.0, 1.0), ambient: float = 0.3,
                      use_color: bool = False) -> torch.Tensor:
        return self._get_renderer().render_shaded(intrinsics, pose, image_shape, light_direction, ambient, use_color)

    def render_depth_colormap(self, intrinsics: torch.Tensor, pose, image_shape) -> torch.Tensor:
        return self._get_renderer().render_depth_colormap(intrinsics, pose, image_shape)

    def render_normal_colormap(self, intrinsics: torch.Tensor, pose, image_shape) -> torch.Tensor:
        return self._get_renderer().render_normal_colormap(intrinsics, pose, image_shape)

    def memory_usage_mb(self) -> float:
        t = self._tsdf
        tensors = (t.block_data, t.block_visible, t.frame_visible, t.lidar_frame_visible, t.block_recycled, self._sites, self._sites_scratch, self._dist_field)
        return sum(x.numel() * x.element_size() for x in tensors) / (1024.0 * 1024.0)

    def get_stats(self) -> dict:
        """``frame_count``, ``total_blocks``, ``visible_blocks`` (ever), ``last_frame_blocks``, ``recycled_blocks`` (by the last
        decay launch), ``block_size``, ``tsdf_grid_shape`` (nz, ny, nx), ``esdf_grid_shape`` (nx, ny, nz), ``memory_mb``"""
        p, t = self._params, self._tsdf
        return {"frame_count": self._frame_count, "total_blocks": p.n_blocks,
                "visible_blocks": int(t.block_visible[: p.n_blocks].sum().item()),
                "last_frame_blocks": int(t.frame_visible[: p.n_blocks].sum().item()), "recycled_blocks": D.recycled_count(t), "block_size": int(p.block_size),
                "tsdf_grid_shape": tuple(self.config.grid_shape), "esdf_grid_shape": self._esdf_shape, "memory_mb": self.memory_usage_mb()}
