"""HIP backend of ``curobo_amd.perception.mapper`` (``csrc/mapper.hip``).  Same conventions as the other backends:
pre-allocated tensors in, mutated in place, current stream."""

from __future__ import annotations

import ctypes as _C
import math
from typing import Optional, Sequence

import torch

from .._lib import check, current_stream, load, ptr
from .perception import _require

ESDF_MAX_AXIS = 1024  #: sites pack 10 bits per axis


class MapperParams(_C.Structure):
    """``curobo_hip_mapper_params`` (see include/curobo_hip.h): read on the host at every launch"""

    _fields_ = [("grid_w", _C.c_int32), ("grid_h", _C.c_int32), ("grid_d", _C.c_int32), ("block_size", _C.c_int32),
                ("nbx", _C.c_int32), ("nby", _C.c_int32), ("nbz", _C.c_int32), ("num_samples", _C.c_int32),
                ("origin", _C.c_float * 3), ("voxel_size", _C.c_float), ("truncation_distance", _C.c_float),
                ("depth_min", _C.c_float), ("depth_max", _C.c_float), ("minimum_tsdf_weight", _C.c_float), ("step_size", _C.c_float)]

    @property
    def n_blocks(self) -> int:
        return int(self.nbx) * int(self.nby) * int(self.nbz)

    @property
    def block_voxels(self) -> int:
        return int(self.block_size) ** 3


def marking_step(block_size: int, voxel_size: float, truncation_distance: float):
    """(step_size, num_samples) of the marking stage (builder_camera_integrate.py: STEP_SIZE, NUM_SAMPLES)"""
    step = block_size * voxel_size / 1.42
    return step, int(math.ceil(2.0 * truncation_distance / step)) + 1


def make_params(grid_shape_zyx: Sequence[int], block_size: int, origin: Sequence[float], voxel_size: float, truncation_distance: float,
                depth_min: float, depth_max: float, minimum_tsdf_weight: float) -> MapperParams:
    """``grid_shape_zyx``: (nz, ny, nx) voxels, as ``MapperCfg.grid_shape``"""
    nz, ny, nx = (int(v) for v in grid_shape_zyx)
    bs = int(block_size)
    step, num_samples = marking_step(bs, voxel_size, truncation_distance)
    p = MapperParams(grid_w=nx, grid_h=ny, grid_d=nz, block_size=bs, nbx=-(-nx // bs), nby=-(-ny // bs), nbz=-(-nz // bs),
                     num_samples=num_samples, voxel_size=voxel_size, truncation_distance=truncation_distance, depth_min=depth_min,
                     depth_max=depth_max, minimum_tsdf_weight=minimum_tsdf_weight, step_size=step)
    p.origin[:] = [float(v) for v in origin]
    return p


def mask_bytes(params: MapperParams) -> int:
    """length of a block mask: one byte per block, rounded up to whole 4-byte words (``mapper_clear_mask`` writes words)"""
    return -(-params.n_blocks // 4) * 4


def _require_map(params: MapperParams, what: str, block_data=None, like=None, **masks) -> None:
    if block_data is not None:
        _require(block_data, "block_data", torch.float16, like)
        if tuple(block_data.shape) != (params.n_blocks, params.block_voxels, 2):
            raise ValueError(f"{what}: block_data must have shape {(params.n_blocks, params.block_voxels, 2)}, got {tuple(block_data.shape)}")
    for name, m in masks.items():
        _require(m, name, torch.uint8, like)
        if m.dim() != 1 or m.numel() < params.n_blocks:
            raise ValueError(f"{what}: {name} must be a vector of at least {params.n_blocks} bytes, got {tuple(m.shape)}")


def _require_cameras(depth, intrinsics, cam_position, cam_quaternion, what: str):
    if depth.dim() != 3:
        raise ValueError(f"{what}: depth must be (num_cameras, H, W), got {tuple(depth.shape)}")
    n, h, w = (int(v) for v in depth.shape)
    for name, t, shape in (("depth", depth, (n, h, w)), ("intrinsics", intrinsics, (n, 3, 3)), ("cam_position", cam_position, (n, 3)),
                           ("cam_quaternion", cam_quaternion, (n, 4))):
        _require(t, name, torch.float32, depth)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} must have shape {shape}, got {tuple(t.shape)}")
    return n, h, w


def mapper_clear_mask(mask: torch.Tensor) -> None:
    """``curobo_hip_mapper_clear_mask``"""
    _require(mask, "mask", torch.uint8)
    check(load().curobo_hip_mapper_clear_mask(ptr(mask), int(mask.numel()), current_stream(mask)))


def mapper_mark_blocks(frame_mask: torch.Tensor, block_mask: torch.Tensor, depth: torch.Tensor, intrinsics: torch.Tensor,
                       cam_position: torch.Tensor, cam_quaternion: torch.Tensor, params: MapperParams) -> None:
    """``curobo_hip_mapper_mark_blocks``: 1 into both masks for every block a sample of this frame falls into"""
    what = "mapper_mark_blocks"
    n, h, w = _require_cameras(depth, intrinsics, cam_position, cam_quaternion, what)
    _require_map(params, what, like=depth, frame_mask=frame_mask, block_mask=block_mask)
    check(load().curobo_hip_mapper_mark_blocks(ptr(frame_mask), ptr(block_mask), ptr(depth), ptr(intrinsics), ptr(cam_position),
                                               ptr(cam_quaternion), _C.addressof(params), n, h, w, current_stream(depth)))


def mapper_integrate(block_data: torch.Tensor, frame_mask: torch.Tensor, depth: torch.Tensor, intrinsics: torch.Tensor,
                     cam_position: torch.Tensor, cam_quaternion: torch.Tensor, params: MapperParams) -> None:
    """``curobo_hip_mapper_integrate``: every voxel of every block of ``frame_mask``"""
    what = "mapper_integrate"
    n, h, w = _require_cameras(depth, intrinsics, cam_position, cam_quaternion, what)
    _require_map(params, what, block_data, like=depth, frame_mask=frame_mask)
    check(load().curobo_hip_mapper_integrate(ptr(block_data), ptr(frame_mask), ptr(depth), ptr(intrinsics), ptr(cam_position),
                                             ptr(cam_quaternion), _C.addressof(params), n, h, w, current_stream(depth)))


def _require_esdf(esdf_origin: torch.Tensor, esdf_voxel_size: torch.Tensor, shape: Sequence[int], what: str, like: torch.Tensor, **cells):
    d, h, w = (int(v) for v in shape)
    _require(esdf_origin, "esdf_origin", torch.float32, like)
    _require(esdf_voxel_size, "esdf_voxel_size", torch.float32, like)
    if esdf_origin.numel() != 3 or esdf_voxel_size.numel() != 1:
        raise ValueError(f"{what}: esdf_origin must hold 3 values and esdf_voxel_size 1")
    for name, (t, dt) in cells.items():
        _require(t, name, dt, like)
        if t.numel() != d * h * w:
            raise ValueError(f"{what}: {name} must hold {d} x {h} x {w} = {d * h * w} cells, got {t.numel()}")
    return d, h, w


def mapper_esdf_seed(sites: torch.Tensor, block_data: torch.Tensor, block_mask: torch.Tensor, esdf_origin: torch.Tensor,
                     esdf_voxel_size: torch.Tensor, params: MapperParams, shape: Sequence[int]) -> None:
    """``curobo_hip_mapper_esdf_seed``: sites int32 [d h w] = the cell's packed coordinates where it is a seed, else -1"""
    what = "mapper_esdf_seed"
    _require_map(params, what, block_data, block_mask=block_mask)
    d, h, w = _require_esdf(esdf_origin, esdf_voxel_size, shape, what, block_data, sites=(sites, torch.int32))
    check(load().curobo_hip_mapper_esdf_seed(ptr(sites), ptr(block_data), ptr(block_mask), ptr(esdf_origin), ptr(esdf_voxel_size),
                                             _C.addressof(params), d, h, w, current_stream(sites)))


def mapper_edt_pass(sites_out: torch.Tensor, sites_in: torch.Tensor, shape: Sequence[int], axis: int) -> None:
    """``curobo_hip_mapper_edt_pass``: one pass (axis 2, then 1, then 0) of the exact nearest-site transform"""
    d, h, w = (int(v) for v in shape)
    for name, t in (("sites_out", sites_out), ("sites_in", sites_in)):
        _require(t, name, torch.int32, sites_in)
        if t.numel() != d * h * w:
            raise ValueError(f"mapper_edt_pass: {name} must hold {d} x {h} x {w} = {d * h * w} cells, got {t.numel()}")
    check(load().curobo_hip_mapper_edt_pass(ptr(sites_out), ptr(sites_in), d, h, w, int(axis), current_stream(sites_in)))


def mapper_edt(sites: torch.Tensor, scratch: torch.Tensor, shape: Sequence[int]) -> torch.Tensor:
    """the three passes: ``sites`` -> ``scratch`` (z) -> ``sites`` (y) -> ``scratch`` (x).  Returns ``scratch``: the nearest sites."""
    mapper_edt_pass(scratch, sites, shape, 2)
    mapper_edt_pass(sites, scratch, shape, 1)
    mapper_edt_pass(scratch, sites, shape, 0)
    return scratch


def mapper_esdf_distance(distance: torch.Tensor, sites: torch.Tensor, block_data: torch.Tensor, block_mask: torch.Tensor,
                         esdf_origin: torch.Tensor, esdf_voxel_size: torch.Tensor, params: MapperParams, shape: Sequence[int]) -> None:
    """``curobo_hip_mapper_esdf_distance``: distance fp16 [d h w], negative inside, 1e4 where there is no site"""
    what = "mapper_esdf_distance"
    _require_map(params, what, block_data, block_mask=block_mask)
    d, h, w = _require_esdf(esdf_origin, esdf_voxel_size, shape, what, block_data, sites=(sites, torch.int32), distance=(distance, torch.float16))
    check(load().curobo_hip_mapper_esdf_distance(ptr(distance), ptr(sites), ptr(block_data), ptr(block_mask), ptr(esdf_origin),
                                                 ptr(esdf_voxel_size), _C.addressof(params), d, h, w, current_stream(distance)))


def mapper_occupied_flags(flags: torch.Tensor, block_data: torch.Tensor, block_mask: torch.Tensor, params: MapperParams,
                          surface_only: bool, sdf_threshold: float) -> None:
    """``curobo_hip_mapper_occupied_flags``: flags uint8 [n_blocks, block_size^3]"""
    what = "mapper_occupied_flags"
    _require_map(params, what, block_data, block_mask=block_mask)
    _require(flags, "flags", torch.uint8, block_data)
    if flags.numel() != params.n_blocks * params.block_voxels:
        raise ValueError(f"{what}: flags must hold {params.n_blocks * params.block_voxels} voxels, got {flags.numel()}")
    check(load().curobo_hip_mapper_occupied_flags(ptr(flags), ptr(block_data), ptr(block_mask), _C.addressof(params), int(bool(surface_only)),
                                                  float(sdf_threshold), current_stream(flags)))


REFERENCE_BLOCK_SIZE = 8  #: the block size the recycle threshold was calibrated at (reference constants.py:55)


def decay_empty_threshold(block_size: int) -> float:
    """the weight sum below which a block is recycled: 0.01 at blocks of 8, scaled by the voxels of a block
    (builder_decay.py:69, :103-105), as the float32 the launch compares with"""
    return float(torch.tensor(0.01 * float(int(block_size) ** 3) / float(REFERENCE_BLOCK_SIZE ** 3), dtype=torch.float32).item())


def mapper_decay(block_data: torch.Tensor, block_mask: torch.Tensor, recycled: torch.Tensor, params: MapperParams, factor_outside: float,
                 factor_inside: float, empty_threshold: float, intrinsics: Optional[torch.Tensor] = None,
                 cam_position: Optional[torch.Tensor] = None, cam_quaternion: Optional[torch.Tensor] = None,
                 image_shape: Sequence[int] = (0, 0)) -> None:
    """``curobo_hip_mapper_decay``: every ever-visible block times ``factor_inside`` where it lies in the union of the cameras'
    frusta (``intrinsics`` [n, 3, 3], ``cam_position`` [n, 3], ``cam_quaternion`` [n, 4] wxyz, ``image_shape`` (H, W), the depth
    range of ``params``), else times ``factor_outside``; without cameras ``factor_outside`` throughout.  A block whose weights then
    sum to less than ``empty_threshold`` is zeroed and leaves ``block_mask``; ``recycled`` uint8 [n_blocks]: 1 for those, else 0."""
    what = "mapper_decay"
    _require_map(params, what, block_data, like=block_data, block_mask=block_mask, recycled=recycled)
    for name, f in (("factor_outside", factor_outside), ("factor_inside", factor_inside)):
        if not 0.0 <= float(f) <= 1.0:
            raise ValueError(f"{what}: {name} must lie in [0, 1], got {f}")
    cameras = (intrinsics, cam_position, cam_quaternion)
    n, h, w = 0, 0, 0
    if any(t is not None for t in cameras):
        if any(t is None for t in cameras):
            raise ValueError(f"{what}: intrinsics, cam_position and cam_quaternion come together")
        n, (h, w) = int(intrinsics.shape[0]), (int(v) for v in image_shape)
        for name, t, shape in (("intrinsics", intrinsics, (n, 3, 3)), ("cam_position", cam_position, (n, 3)), ("cam_quaternion", cam_quaternion, (n, 4))):
            _require(t, name, torch.float32, block_data)
            if tuple(t.shape) != shape:
                raise ValueError(f"{what}: {name} must have shape {shape}, got {tuple(t.shape)}")
        if n <= 0 or h <= 0 or w <= 0:
            raise ValueError(f"{what}: need at least one camera and a positive image_shape, got {n} cameras and {(h, w)}")
    check(load().curobo_hip_mapper_decay(ptr(block_data), ptr(block_mask), ptr(recycled), ptr(intrinsics), ptr(cam_position), ptr(cam_quaternion),
                                         n, h, w, float(factor_outside), float(factor_inside), float(empty_threshold), _C.addressof(params),
                                         current_stream(block_data)))


def _require_lidars(position, quaternion, valid_range, elevation_range, what: str, like: torch.Tensor) -> int:
    """the per-lidar arrays ``lidar_position`` [n, 3], ``lidar_quaternion`` [n, 4] wxyz, ``valid_range`` [n, 2], ``elevation_range`` [n, 2]"""
    if position is None or position.dim() != 2:
        raise ValueError(f"{what}: lidar_position must have shape (num_lidars, 3), got {None if position is None else tuple(position.shape)}")
    n = int(position.shape[0])
    for name, t, shape in (("lidar_position", position, (n, 3)), ("lidar_quaternion", quaternion, (n, 4)), ("valid_range", valid_range, (n, 2)),
                           ("elevation_range", elevation_range, (n, 2))):
        if t is None:
            raise ValueError(f"{what}: {name} is required")
        _require(t, name, torch.float32, like)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} must have shape {shape}, got {tuple(t.shape)}")
    if n <= 0:
        raise ValueError(f"{what}: need at least one lidar")
    return n


def _require_range(range_image, position, quaternion, valid_range, elevation_range, what: str):
    if range_image.dim() != 3:
        raise ValueError(f"{what}: range_image must be (num_lidars, H, W), got {tuple(range_image.shape)}")
    _require(range_image, "range_image", torch.float32)
    n, h, w = (int(v) for v in range_image.shape)
    if _require_lidars(position, quaternion, valid_range, elevation_range, what, range_image) != n:
        raise ValueError(f"{what}: lidar_position holds {int(position.shape[0])} lidars, range_image {n}")
    return n, h, w


def mapper_lidar_mark_blocks(lidar_mask: torch.Tensor, frame_mask: torch.Tensor, block_mask: torch.Tensor, range_image: torch.Tensor,
                             lidar_position: torch.Tensor, lidar_quaternion: torch.Tensor, valid_range: torch.Tensor,
                             elevation_range: torch.Tensor, params: MapperParams) -> None:
    """``curobo_hip_mapper_lidar_mark_blocks``: 1 into the three masks for every block a sample of this frame's range images
    ``(num_lidars, H, W)`` falls into; ``valid_range`` [n, 2] metres, ``elevation_range`` [n, 2] radians"""
    what = "mapper_lidar_mark_blocks"
    n, h, w = _require_range(range_image, lidar_position, lidar_quaternion, valid_range, elevation_range, what)
    _require_map(params, what, like=range_image, lidar_mask=lidar_mask, frame_mask=frame_mask, block_mask=block_mask)
    check(load().curobo_hip_mapper_lidar_mark_blocks(ptr(lidar_mask), ptr(frame_mask), ptr(block_mask), ptr(range_image), ptr(lidar_position),
                                                     ptr(lidar_quaternion), ptr(valid_range), ptr(elevation_range), _C.addressof(params), n, h, w,
                                                     current_stream(range_image)))


def mapper_lidar_integrate(block_data: torch.Tensor, lidar_mask: torch.Tensor, range_image: torch.Tensor, lidar_position: torch.Tensor,
                           lidar_quaternion: torch.Tensor, valid_range: torch.Tensor, elevation_range: torch.Tensor, params: MapperParams,
                           linear_max_diff_m: float, nearest_max_dist_m: float) -> None:
    """``curobo_hip_mapper_lidar_integrate``: every voxel of every block of ``lidar_mask``; the two interpolation guards in metres"""
    what = "mapper_lidar_integrate"
    n, h, w = _require_range(range_image, lidar_position, lidar_quaternion, valid_range, elevation_range, what)
    _require_map(params, what, block_data, like=range_image, lidar_mask=lidar_mask)
    for name, v in (("linear_max_diff_m", linear_max_diff_m), ("nearest_max_dist_m", nearest_max_dist_m)):
        if not float(v) > 0.0:
            raise ValueError(f"{what}: {name} must be positive, got {v}")
    check(load().curobo_hip_mapper_lidar_integrate(ptr(block_data), ptr(lidar_mask), ptr(range_image), ptr(lidar_position), ptr(lidar_quaternion),
                                                   ptr(valid_range), ptr(elevation_range), _C.addressof(params), n, h, w,
                                                   float(linear_max_diff_m), float(nearest_max_dist_m), current_stream(range_image)))


def mapper_decay_sensors(block_data: torch.Tensor, block_mask: torch.Tensor, recycled: torch.Tensor, params: MapperParams,
                         factor_outside: float, factor_inside: float, empty_threshold: float, intrinsics: Optional[torch.Tensor] = None,
                         cam_position: Optional[torch.Tensor] = None, cam_quaternion: Optional[torch.Tensor] = None,
                         image_shape: Sequence[int] = (0, 0), lidar_position: Optional[torch.Tensor] = None,
                         lidar_quaternion: Optional[torch.Tensor] = None, lidar_valid_range: Optional[torch.Tensor] = None,
                         lidar_elevation_range: Optional[torch.Tensor] = None, lidar_height: int = 0) -> None:
    """``curobo_hip_mapper_decay_sensors``: ``mapper_decay`` over the union of the cameras' frusta and the lidars' (``lidar_position``
    [n, 3], ``lidar_quaternion`` [n, 4] wxyz, ``lidar_valid_range`` [n, 2] metres, ``lidar_elevation_range`` [n, 2] radians,
    ``lidar_height`` the rows of the range image); either set may be left out"""
    what = "mapper_decay_sensors"
    _require_map(params, what, block_data, like=block_data, block_mask=block_mask, recycled=recycled)
    for name, f in (("factor_outside", factor_outside), ("factor_inside", factor_inside)):
        if not 0.0 <= float(f) <= 1.0:
            raise ValueError(f"{what}: {name} must lie in [0, 1], got {f}")
    cameras = (intrinsics, cam_position, cam_quaternion)
    n, h, w = 0, 0, 0
    if any(t is not None for t in cameras):
        if any(t is None for t in cameras):
            raise ValueError(f"{what}: intrinsics, cam_position and cam_quaternion come together")
        n, (h, w) = int(intrinsics.shape[0]), (int(v) for v in image_shape)
        for name, t, shape in (("intrinsics", intrinsics, (n, 3, 3)), ("cam_position", cam_position, (n, 3)), ("cam_quaternion", cam_quaternion, (n, 4))):
            _require(t, name, torch.float32, block_data)
            if tuple(t.shape) != shape:
                raise ValueError(f"{what}: {name} must have shape {shape}, got {tuple(t.shape)}")
        if n <= 0 or h <= 0 or w <= 0:
            raise ValueError(f"{what}: need at least one camera and a positive image_shape, got {n} cameras and {(h, w)}")
    lidars = (lidar_position, lidar_quaternion, lidar_valid_range, lidar_elevation_range)
    n_lidars = 0
    if any(t is not None for t in lidars):
        n_lidars = _require_lidars(*lidars, what, block_data)
        if int(lidar_height) <= 0:
            raise ValueError(f"{what}: lidar_height must be positive, got {lidar_height}")
    check(load().curobo_hip_mapper_decay_sensors(ptr(block_data), ptr(block_mask), ptr(recycled), ptr(intrinsics), ptr(cam_position),
                                                 ptr(cam_quaternion), n, h, w, ptr(lidar_position), ptr(lidar_quaternion), ptr(lidar_valid_range),
                                                 ptr(lidar_elevation_range), n_lidars, int(lidar_height) if n_lidars else 0,
                                                 float(factor_outside), float(factor_inside), float(empty_threshold), _C.addressof(params),
                                                 current_stream(block_data)))


def _require_mesh(params: MapperParams, what: str, block_list: torch.Tensor, **per_voxel) -> int:
    """``block_list`` int32 [n_slots] and the per-voxel arrays [n_slots * block_size^3] (``(tensor, dtype, width)``); returns n_slots"""
    _require(block_list, "block_list", torch.int32)
    n_slots = int(block_list.numel())
    if block_list.dim() != 1 or not 0 < n_slots <= params.n_blocks:
        raise ValueError(f"{what}: block_list must be a vector of 1..{params.n_blocks} blocks, got {tuple(block_list.shape)}")
    if n_slots * params.block_voxels * 5 >= 2 ** 31:
        raise ValueError(f"{what}: {n_slots} visible blocks of {params.block_voxels} voxels may hold 2^31 triangles or more; indices are int32")
    for name, (t, dt, width) in per_voxel.items():
        _require(t, name, dt, block_list)
        if t.numel() != n_slots * params.block_voxels * width:
            raise ValueError(f"{what}: {name} must hold {n_slots} x {params.block_voxels} x {width} values, got {t.numel()}")
    return n_slots


def _require_rows(what: str, like: torch.Tensor, **rows) -> None:
    """``(tensor, dtype, rows, width)``: contiguous, on ``like``'s device, of exactly that many values"""
    for name, (t, dt, n, width) in rows.items():
        _require(t, name, dt, like)
        if t.numel() != n * width:
            raise ValueError(f"{what}: {name} must hold {n} x {width} values, got {t.numel()}")


def mapper_mesh_classify(cube_case: torch.Tensor, vert_count: torch.Tensor, tri_count: torch.Tensor, block_data: torch.Tensor,
                         block_mask: torch.Tensor, block_list: torch.Tensor, table: torch.Tensor, params: MapperParams, level: float,
                         surface_only: bool) -> None:
    """``curobo_hip_mapper_mesh_classify``: per voxel of the listed blocks the case byte (0: no surface cube), the vertices it
    owns (0..3) and the triangles of its table row (0..5); ``table`` int8 [256, 16]"""
    what = "mapper_mesh_classify"
    _require_map(params, what, block_data, block_mask=block_mask)
    _require_mesh(params, what, block_list, cube_case=(cube_case, torch.uint8, 1), vert_count=(vert_count, torch.uint8, 1),
                  tri_count=(tri_count, torch.uint8, 1))
    _require_rows(what, block_list, table=(table, torch.int8, 256, 16))
    check(load().curobo_hip_mapper_mesh_classify(ptr(cube_case), ptr(vert_count), ptr(tri_count), ptr(block_data), ptr(block_mask), ptr(block_list),
                                                 int(block_list.numel()), ptr(table), _C.addressof(params), float(level),
                                                 int(bool(surface_only)), current_stream(cube_case)))


def mapper_mesh_vertices(vertices: torch.Tensor, normals: torch.Tensor, vert_ids: torch.Tensor, vert_count: torch.Tensor,
                         vert_offset: torch.Tensor, block_data: torch.Tensor, block_mask: torch.Tensor, block_list: torch.Tensor,
                         params: MapperParams, level: float, refine_iterations: int) -> None:
    """``curobo_hip_mapper_mesh_vertices``: vertices, normals float32 [V, 3] at the offsets ``vert_offset`` (the exclusive prefix
    sum of ``vert_count``, V its total), and the voxels' vertex ids int32 [n_slots * block_size^3, 3]"""
    what = "mapper_mesh_vertices"
    _require_map(params, what, block_data, block_mask=block_mask)
    _require_mesh(params, what, block_list, vert_ids=(vert_ids, torch.int32, 3), vert_count=(vert_count, torch.uint8, 1),
                  vert_offset=(vert_offset, torch.int32, 1))
    n = int(vertices.shape[0])
    _require_rows(what, block_list, vertices=(vertices, torch.float32, n, 3), normals=(normals, torch.float32, n, 3))
    check(load().curobo_hip_mapper_mesh_vertices(ptr(vertices), ptr(normals), ptr(vert_ids), n, ptr(vert_count), ptr(vert_offset), ptr(block_data),
                                                 ptr(block_mask), ptr(block_list), int(block_list.numel()), _C.addressof(params), float(level),
                                                 int(refine_iterations), current_stream(vertices)))


def mapper_mesh_triangles(raw_triangles: torch.Tensor, keep: torch.Tensor, cube_case: torch.Tensor, tri_count: torch.Tensor,
                          tri_offset: torch.Tensor, vert_ids: torch.Tensor, vertices: torch.Tensor, block_list: torch.Tensor,
                          block_slot: torch.Tensor, table: torch.Tensor, edge_owner: torch.Tensor, params: MapperParams) -> None:
    """``curobo_hip_mapper_mesh_triangles``: every table triangle of every surface cube, int32 [n_raw, 3] with -1 for a missing
    vertex, and ``keep`` uint8 [n_raw]; ``block_slot`` int32 [n_blocks], ``edge_owner`` int8 [12, 4]"""
    what = "mapper_mesh_triangles"
    _require_mesh(params, what, block_list, cube_case=(cube_case, torch.uint8, 1), tri_count=(tri_count, torch.uint8, 1),
                  tri_offset=(tri_offset, torch.int32, 1), vert_ids=(vert_ids, torch.int32, 3))
    n_raw, n_vertices = int(raw_triangles.shape[0]), int(vertices.shape[0])
    _require_rows(what, block_list, raw_triangles=(raw_triangles, torch.int32, n_raw, 3), keep=(keep, torch.uint8, n_raw, 1),
                  vertices=(vertices, torch.float32, n_vertices, 3), block_slot=(block_slot, torch.int32, params.n_blocks, 1),
                  table=(table, torch.int8, 256, 16), edge_owner=(edge_owner, torch.int8, 12, 4))
    check(load().curobo_hip_mapper_mesh_triangles(ptr(raw_triangles), ptr(keep), n_raw, ptr(cube_case), ptr(tri_count), ptr(tri_offset),
                                                  ptr(vert_ids), ptr(vertices), n_vertices, ptr(block_list), ptr(block_slot),
                                                  int(block_list.numel()), ptr(table), ptr(edge_owner), _C.addressof(params),
                                                  current_stream(raw_triangles)))


def mapper_mesh_compact(triangles: torch.Tensor, raw_triangles: torch.Tensor, keep: torch.Tensor, keep_offset: torch.Tensor) -> None:
    """``curobo_hip_mapper_mesh_compact``: the raw triangles with ``keep`` set, in their order, to int32 [n, 3]; ``keep_offset`` int32:
    the exclusive prefix sum of ``keep``, n its total"""
    what = "mapper_mesh_compact"
    n_raw, n = int(raw_triangles.shape[0]), int(triangles.shape[0])
    _require_rows(what, raw_triangles, triangles=(triangles, torch.int32, n, 3), raw_triangles=(raw_triangles, torch.int32, n_raw, 3),
                  keep=(keep, torch.uint8, n_raw, 1), keep_offset=(keep_offset, torch.int32, n_raw, 1))
    check(load().curobo_hip_mapper_mesh_compact(ptr(triangles), n, ptr(raw_triangles), ptr(keep), ptr(keep_offset), n_raw,
                                                current_stream(triangles)))


# ---------------------------------------------------------------------------------------------------- raycast (csrc/mapper_raycast.hip)
def _require_camera(intrinsics: torch.Tensor, position: torch.Tensor, quaternion: torch.Tensor, what: str, like: torch.Tensor) -> None:
    for name, t, n in (("intrinsics", intrinsics, 9), ("position", position, 3), ("quaternion", quaternion, 4)):
        _require(t, name, torch.float32, like)
        if t.numel() != n:
            raise ValueError(f"{what}: {name} must hold {n} values, got {tuple(t.shape)}")


def mapper_raycast(hit_points: torch.Tensor, hit_normals: torch.Tensor, hit_depths: torch.Tensor, hit_mask: torch.Tensor,
                   intrinsics: torch.Tensor, position: torch.Tensor, quaternion: torch.Tensor, block_data: torch.Tensor,
                   block_mask: torch.Tensor, params: MapperParams, minimum_tsdf_weight: float, depth_minimum_distance: float,
                   depth_maximum_distance: float, image_shape: Sequence[int], accelerated: bool, z_depth: bool = False) -> None:
    """``curobo_hip_mapper_raycast``: one ray per pixel of an ``(H, W)`` image from the camera ``intrinsics`` [3, 3], ``position`` [3],
    ``quaternion`` [4] wxyz (device tensors) -> hit_points, hit_normals float32 [H W, 3], hit_depths float32 [H W] (range along the
    ray; ``z_depth``: along the camera's axis), hit_mask uint8 [H W], all zero on a miss"""
    what = "mapper_raycast"
    h, w = (int(v) for v in image_shape)
    _require_map(params, what, block_data, block_mask=block_mask)
    _require_camera(intrinsics, position, quaternion, what, block_data)
    _require_rows(what, block_data, hit_points=(hit_points, torch.float32, h * w, 3), hit_normals=(hit_normals, torch.float32, h * w, 3),
                  hit_depths=(hit_depths, torch.float32, h * w, 1), hit_mask=(hit_mask, torch.uint8, h * w, 1))
    check(load().curobo_hip_mapper_raycast(ptr(hit_points), ptr(hit_normals), ptr(hit_depths), ptr(hit_mask), ptr(intrinsics), ptr(position),
                                           ptr(quaternion), ptr(block_data), ptr(block_mask), _C.addressof(params), float(minimum_tsdf_weight),
                                           float(depth_minimum_distance), float(depth_maximum_distance), h, w, int(bool(accelerated)),
                                           int(bool(z_depth)), current_stream(hit_depths)))


def ray_align_samples(image_shape: Sequence[int], stride: int, n_samples_per_ray: int) -> int:
    """how many samples ``mapper_ray_align`` evaluates: ceil(H / stride) ceil(W / stride) n_samples_per_ray -- the ``n_points`` of
    ``pose_sdf_ws_bytes`` and ``pose_lm_step`` for its workspace"""
    h, w = (int(v) for v in image_shape)
    return -(-h // int(stride)) * -(-w // int(stride)) * int(n_samples_per_ray)


def mapper_ray_align(workspace: torch.Tensor, depth: torch.Tensor, intrinsics: torch.Tensor, position: torch.Tensor,
                     quaternion: torch.Tensor, block_data: torch.Tensor, block_mask: torch.Tensor, params: MapperParams,
                     minimum_tsdf_weight: float, depth_minimum_distance: float, depth_maximum_distance: float, distance_threshold: float,
                     stride: int, n_samples_per_ray: int) -> None:
    """``curobo_hip_mapper_ray_align``: the along-ray SDF residuals of ``depth`` [H, W] at the pose ``position`` [3] / ``quaternion`` [4]
    wxyz on the device -> one row of partial sums per workgroup of 256 samples in ``workspace``, for ``pose_lm_step``"""
    what = "mapper_ray_align"
    if depth.dim() != 2:
        raise ValueError(f"{what}: depth must be (H, W), got {tuple(depth.shape)}")
    _require(depth, "depth", torch.float32)
    _require_map(params, what, block_data, like=depth, block_mask=block_mask)
    _require_camera(intrinsics, position, quaternion, what, depth)
    if not workspace.is_contiguous() or workspace.device != depth.device:
        raise ValueError(f"{what}: workspace must be a contiguous tensor on depth's device")
    check(load().curobo_hip_mapper_ray_align(ptr(workspace), int(workspace.numel() * workspace.element_size()), ptr(depth), ptr(intrinsics),
                                             ptr(position), ptr(quaternion), ptr(block_data), ptr(block_mask), _C.addressof(params),
                                             float(minimum_tsdf_weight), float(depth_minimum_distance), float(depth_maximum_distance),
                                             float(distance_threshold), int(depth.shape[0]), int(depth.shape[1]), int(stride),
                                             int(n_samples_per_ray), current_stream(depth)))
