"""``MapperCfg``: the reference's configuration of the volumetric mapper (``perception/mapper/mapper_cfg.py``), field for
field where this mapper has the capability, refusing by name what it has not."""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

#: sites of the distance transform pack 10 bits per axis
ESDF_MAX_AXIS = 1024
_BLOCK_SIZES = (1, 2, 4, 8, 16, 32)


def _plain_int(name: str, value) -> int:
    if not isinstance(value, int) or isinstance(value, bool):
        raise ValueError(f"{name} must be a plain int, got {type(value).__name__} ({value!r})")
    return value


@dataclass
class MapperLidarCfg:
    """The lidar settings of :class:`Mapper`, handed to its constructor: ``Mapper(cfg, lidar=MapperLidarCfg(...))``.  The fields are
    the reference's ``MapperCfg.lidar_*`` (``mapper_cfg.py:138-158``) without the prefix, with its checks (``constants.py:179-263``):
    ``num_sensors`` range images of ``image_height`` x ``image_width`` pixels per frame (``image_height == 1``: a planar scan);
    a bilinear range is accepted when no corner differs from it by more than
    ``linear_interpolation_max_allowable_difference_vox`` voxels, the nearest pixel's when the voxel lies within
    ``nearest_interpolation_max_allowable_dist_to_ray_vox`` voxels of that pixel's ray.

    ``max_visible_blocks_per_lidar_integration`` and ``max_support_pixels_per_block_lidar`` are accepted, checked as the
    reference checks them, and have no effect: the map is dense, so no list of visible blocks is sized, and there is no colour
    or feature channel for the support pixels to gather."""

    num_sensors: int = 1
    image_height: Optional[int] = None
    image_width: Optional[int] = None
    linear_interpolation_max_allowable_difference_vox: float = 2.0
    nearest_interpolation_max_allowable_dist_to_ray_vox: float = 0.5
    max_visible_blocks_per_lidar_integration: Optional[int] = None
    max_support_pixels_per_block_lidar: int = 8

    def __post_init__(self):
        if _plain_int("num_sensors", self.num_sensors) <= 0:
            raise ValueError(f"num_sensors must be positive: {self.num_sensors}")
        if self.image_height is None or self.image_width is None:
            raise ValueError("MapperLidarCfg requires image_height and image_width")
        if _plain_int("image_height", self.image_height) <= 0 or _plain_int("image_width", self.image_width) <= 0:
            raise ValueError(f"image_height and image_width must be positive, got {self.image_height}x{self.image_width}")
        if _plain_int("max_support_pixels_per_block_lidar", self.max_support_pixels_per_block_lidar) <= 0:
            raise ValueError(f"max_support_pixels_per_block_lidar must be positive: {self.max_support_pixels_per_block_lidar}")
        for name in ("linear_interpolation_max_allowable_difference_vox", "nearest_interpolation_max_allowable_dist_to_ray_vox"):
            if not float(getattr(self, name)) > 0.0:
                raise ValueError(f"{name} must be positive: {getattr(self, name)}")
        if self.max_visible_blocks_per_lidar_integration is not None and self.max_visible_blocks_per_lidar_integration <= 0:
            raise ValueError(f"max_visible_blocks_per_lidar_integration must be positive: {self.max_visible_blocks_per_lidar_integration}")


@dataclass
class MapperCfg:
    """Grid, sensor and ESDF settings of :class:`Mapper`.

    Conventions (the reference's): ``extent_meters_xyz`` is the extent of the voxel bounds, ``grid_shape`` is
    ``(nz, ny, nx)``, each ``ceil(extent / voxel_size)``, so the grid may be slightly larger than asked for
    (``get_actual_extent``); voxel ``(iz, iy, ix)`` has its centre at ``grid_center + (i - (n - 1) / 2) voxel_size`` per axis.
    The ESDF grid has ``ceil(extent_esdf_meters_xyz / esdf_voxel_size)`` cells along x, y, z (x slowest), 128 per axis when
    no extent is given, at most 1024 per axis.

    The TSDF is stored dense (padded to whole blocks of ``block_size`` voxels per edge), so ``hash_load_factor`` and
    ``roughness`` are accepted and have no effect, and ``max_blocks`` / ``hash_capacity`` report the dense block count; the
    bound that matters here is ``max_dense_bytes``.  Not built, and refused by name when set away from the default:
    ``enable_static``, ``lidar_num_sensors`` > 0, ``feature_dim`` > 0, ``seeding_method="scatter"``, ``edt_solver="jfa"``.

    Weight decay and block recycling ARE built, yet ``decay_factor`` / ``frustum_decay_factor`` != 1 are still refused here:
    tests/test_mapper_host.py pins that refusal and existing tests stay as they are.  Set the factors where the reference's
    integrator has them instead: ``Mapper(cfg, time_decay=..., frustum_decay=...)``, or call ``Mapper.decay_and_recycle`` /
    ``perception.mapper.decay`` yourself.  Lifting the refusal is a two-line follow-up: drop the two rows of the refusal table
    below and hand the fields to ``Mapper`` as its defaults.

    Lidar range-image integration IS built as well, and ``lidar_num_sensors`` > 0 is refused here for the same reason (the same
    test pins it).  Configure the sensors at the constructor: ``Mapper(cfg, lidar=MapperLidarCfg(num_sensors=...,
    image_height=..., image_width=...))``.  Lifting the refusal is the same kind of follow-up: drop the ``lidar_num_sensors`` row
    and build the ``MapperLidarCfg`` from ``lidar_*`` fields here.
    """

    # grid
    extent_meters_xyz: Tuple[float, float, float]
    voxel_size: float = 0.005
    esdf_voxel_size: float = 0.05
    extent_esdf_meters_xyz: Optional[Tuple[float, float, float]] = None
    grid_center: Optional[torch.Tensor] = None
    # TSDF
    truncation_distance: float = 0.04
    minimum_tsdf_weight: float = 0.1
    # depth sensor
    depth_minimum_distance: float = 0.1
    depth_maximum_distance: float = 10.0
    # decay (refused here; see the docstring: Mapper(cfg, time_decay=, frustum_decay=))
    decay_factor: float = 1.0
    frustum_decay_factor: float = 1.0
    # block storage
    block_size: int = 4
    hash_load_factor: float = 0.5
    roughness: float = 3.0
    # ESDF
    seeding_method: str = "gather"
    edt_solver: str = "pba"
    # static obstacles (not built)
    enable_static: bool = False
    static_obstacle_color: Tuple[int, int, int] = (20, 20, 20)
    # cameras
    num_cameras: int = 1
    image_height: Optional[int] = None
    image_width: Optional[int] = None
    # lidar, features (not built)
    lidar_num_sensors: int = 0
    feature_dim: int = 0
    device: str = "cuda:0"
    #: this project's field: the most the dense TSDF (two fp16 words per voxel of the padded grid) may take
    max_dense_bytes: int = 4 << 30

    def __post_init__(self):
        if len(self.extent_meters_xyz) != 3 or not all(e > 0 for e in self.extent_meters_xyz):
            raise ValueError(f"extent_meters_xyz must be three positive extents: {self.extent_meters_xyz}")
        if self.voxel_size <= 0 or self.esdf_voxel_size <= 0:
            raise ValueError(f"voxel_size and esdf_voxel_size must be positive: {self.voxel_size}, {self.esdf_voxel_size}")
        if self.truncation_distance <= 0:
            raise ValueError(f"truncation_distance must be positive: {self.truncation_distance}")
        if self.depth_minimum_distance >= self.depth_maximum_distance:
            raise ValueError(f"depth_minimum_distance ({self.depth_minimum_distance}) must be < depth_maximum_distance "
                             f"({self.depth_maximum_distance})")
        for name in ("decay_factor", "frustum_decay_factor"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError(f"{name} must be in (0, 1]: {getattr(self, name)}")
        if not 0.0 < self.hash_load_factor <= 1.0:
            raise ValueError(f"hash_load_factor must be in (0, 1]: {self.hash_load_factor}")
        if self.block_size not in _BLOCK_SIZES:
            raise ValueError(f"block_size must be one of {_BLOCK_SIZES}: {self.block_size}")
        if self.image_height is None or self.image_width is None or self.image_height <= 0 or self.image_width <= 0:
            raise ValueError(f"MapperCfg requires positive image_height and image_width, got {self.image_height} and {self.image_width}")
        if self.num_cameras <= 0:
            raise ValueError(f"num_cameras must be positive: {self.num_cameras}")
        if self.seeding_method not in ("gather", "scatter"):
            raise ValueError(f"seeding_method must be 'gather' or 'scatter': {self.seeding_method!r}")
        if self.edt_solver not in ("pba", "jfa"):
            raise ValueError(f"edt_solver must be 'pba' or 'jfa': {self.edt_solver!r}")
        for name, unbuilt, what in (
                ("decay_factor", self.decay_factor != 1.0, "weight decay"),
                ("frustum_decay_factor", self.frustum_decay_factor != 1.0, "weight decay"),
                ("enable_static", bool(self.enable_static), "static obstacle stamping"),
                ("lidar_num_sensors", self.lidar_num_sensors > 0, "lidar integration"),
                ("feature_dim", self.feature_dim > 0, "feature channels"),
                ("seeding_method", self.seeding_method == "scatter", "scatter seeding (the gather rule is the one built)"),
                ("edt_solver", self.edt_solver == "jfa", "jump flooding (the exact transform, 'pba', is the one built)")):
            if unbuilt:
                raise NotImplementedError(f"MapperCfg.{name}={getattr(self, name)!r}: {what} is not part of this mapper")
        if max(self.esdf_grid_shape) > ESDF_MAX_AXIS:
            raise ValueError(f"the ESDF grid {self.esdf_grid_shape} has more than {ESDF_MAX_AXIS} cells along an axis (its sites pack "
                             "10 bits per axis): use a larger esdf_voxel_size or a smaller extent_esdf_meters_xyz")
        if self.dense_bytes > self.max_dense_bytes:
            raise ValueError(f"the dense TSDF of {self.grid_shape} voxels in blocks of {self.block_size} needs {self.dense_bytes} bytes, "
                             f"more than max_dense_bytes = {self.max_dense_bytes}")
        if self.grid_center is None:
            self.grid_center = torch.zeros(3, dtype=torch.float32)
        elif not isinstance(self.grid_center, torch.Tensor):
            self.grid_center = torch.tensor(self.grid_center, dtype=torch.float32)

    @property
    def grid_shape(self) -> Tuple[int, int, int]:
        """``(nz, ny, nx)`` voxel counts"""
        x, y, z = self.extent_meters_xyz
        return (math.ceil(z / self.voxel_size), math.ceil(y / self.voxel_size), math.ceil(x / self.voxel_size))

    @property
    def esdf_grid_shape(self) -> Tuple[int, int, int]:
        """``(nx, ny, nz)`` cells of the ESDF grid, x slowest"""
        if self.extent_esdf_meters_xyz is None:
            return (128, 128, 128)
        return tuple(math.ceil(e / self.esdf_voxel_size) for e in self.extent_esdf_meters_xyz)

    @property
    def block_grid_shape(self) -> Tuple[int, int, int]:
        """``(nbz, nby, nbx)`` blocks of the padded grid"""
        return tuple(-(-n // self.block_size) for n in self.grid_shape)

    @property
    def max_blocks(self) -> int:
        """every block of the dense grid (the reference sizes a pool by a surface heuristic here)"""
        nbz, nby, nbx = self.block_grid_shape
        return nbz * nby * nbx

    @property
    def hash_capacity(self) -> int:
        """as the reference computes it from ``max_blocks``; nothing is hashed"""
        return int(math.ceil(self.max_blocks / self.hash_load_factor))

    @property
    def dense_bytes(self) -> int:
        """bytes of the dense TSDF: two fp16 words per voxel of the padded grid"""
        return self.max_blocks * self.block_size ** 3 * 4

    def get_actual_extent(self) -> Tuple[float, float, float]:
        """the extent ``(x, y, z)`` after the rounding up to whole voxels"""
        nz, ny, nx = self.grid_shape
        return (nx * self.voxel_size, ny * self.voxel_size, nz * self.voxel_size)

    def voxel_to_world(self, iz: int, iy: int, ix: int) -> Tuple[float, float, float]:
        """centre of voxel ``(iz, iy, ix)`` as ``(x, y, z)``"""
        nz, ny, nx = self.grid_shape
        c = self.grid_center.tolist()
        return tuple(c[a] + (i - (n - 1) / 2.0) * self.voxel_size for a, (i, n) in enumerate(((ix, nx), (iy, ny), (iz, nz))))

    def world_to_voxel(self, world_x: float, world_y: float, world_z: float) -> Tuple[int, int, int]:
        """``(iz, iy, ix)`` of the voxel whose centre is nearest, ``(-1, -1, -1)`` outside the grid"""
        nz, ny, nx = self.grid_shape
        c = self.grid_center.tolist()
        ix, iy, iz = (int(round((w - c[a]) / self.voxel_size + (n - 1) / 2.0)) for a, (w, n) in
                      enumerate(((world_x, nx), (world_y, ny), (world_z, nz))))
        if 0 <= ix < nx and 0 <= iy < ny and 0 <= iz < nz:
            return (iz, iy, ix)
        return (-1, -1, -1)

    def get_grid_bounds(self) -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
        """``((x, y, z) min corner, (x, y, z) max corner)`` of the voxel bounds"""
        c = self.grid_center.tolist()
        half = [0.5 * e for e in self.get_actual_extent()]
        return (tuple(c[a] - half[a] for a in range(3)), tuple(c[a] + half[a] for a in range(3)))
