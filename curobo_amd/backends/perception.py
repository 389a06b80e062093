"""HIP backend of ``curobo_amd.perception`` (``csrc/perception.hip``: filter_depth_kernel and robot_mask_kernel).  Same
conventions as the other backends: pre-allocated tensors in, mutated in place, current stream."""

from __future__ import annotations

from typing import Optional

import torch

from .._lib import check, current_stream, load, ptr

#: arithmetic modes of ``robot_mask`` (``bf16_ops`` argument of ``curobo_hip_robot_mask``)
MASK_FP32, MASK_BF16_OPS = 0, 1


def _require(t: Optional[torch.Tensor], name: str, dtype: torch.dtype, like: Optional[torch.Tensor] = None) -> None:
    if t is None:
        return
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor, got {t.dtype} with strides {tuple(t.stride())}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, expected {like.device}")


def filter_depth(depth_out: torch.Tensor, valid_mask_out: torch.Tensor, depth_in: torch.Tensor, temp_a: Optional[torch.Tensor],
                 temp_b: Optional[torch.Tensor], depth_minimum_distance: float, depth_maximum_distance: float,
                 enable_flying_pixel: bool, flying_tolerance: float, bilateral_kernel_size: int, sigma_spatial_sq2: float,
                 sigma_depth_sq2: float) -> None:
    """``curobo_hip_filter_depth``: (B, H, W) fp32 depth -> depth_out fp32 (rejected pixels 0), valid_mask_out uint8.
    ``bilateral_kernel_size`` 0 switches smoothing off; sizes >= 7 need the two (B, H, W) fp32 scratch images."""
    if depth_in.dim() != 3:
        raise ValueError(f"filter_depth: depth must be (B, H, W), got {tuple(depth_in.shape)}")
    _require(depth_in, "depth_in", torch.float32)
    _require(depth_out, "depth_out", torch.float32, depth_in)
    _require(valid_mask_out, "valid_mask_out", torch.uint8, depth_in)
    for name, t in (("depth_out", depth_out), ("valid_mask_out", valid_mask_out), ("temp_a", temp_a), ("temp_b", temp_b)):
        if t is not None and tuple(t.shape) != tuple(depth_in.shape):
            raise ValueError(f"filter_depth: {name} has shape {tuple(t.shape)}, depth {tuple(depth_in.shape)}")
    _require(temp_a, "temp_a", torch.float32, depth_in)
    _require(temp_b, "temp_b", torch.float32, depth_in)
    B, H, W = (int(v) for v in depth_in.shape)
    check(load().curobo_hip_filter_depth(
        ptr(depth_out), ptr(valid_mask_out), ptr(depth_in), ptr(temp_a), ptr(temp_b), B, H, W, float(depth_minimum_distance),
        float(depth_maximum_distance), int(bool(enable_flying_pixel)), float(flying_tolerance), int(bilateral_kernel_size),
        float(sigma_spatial_sq2), float(sigma_depth_sq2), current_stream(depth_in)))


def robot_mask(mask_out: torch.Tensor, depth_out: torch.Tensor, depth: torch.Tensor, projection_rays: torch.Tensor,
               camera_position: torch.Tensor, camera_quaternion: torch.Tensor, robot_spheres: torch.Tensor,
               distance_threshold: float, mode: int = MASK_FP32) -> None:
    """``curobo_hip_robot_mask``: depth (B, H, W), projection_rays (B or 1, H W, 3), camera pose (B or 1, 3) / (B or 1, 4) wxyz,
    robot_spheres (B or 1, S, 4) -> mask_out uint8 (B, H, W), depth_out = depth with the robot's pixels set to 0."""
    if depth.dim() != 3:
        raise ValueError(f"robot_mask: depth must be (B, H, W), got {tuple(depth.shape)}")
    B, H, W = (int(v) for v in depth.shape)
    _require(depth, "depth", torch.float32)
    for name, t in (("depth_out", depth_out), ("projection_rays", projection_rays), ("camera_position", camera_position),
                    ("camera_quaternion", camera_quaternion), ("robot_spheres", robot_spheres)):
        _require(t, name, torch.float32, depth)
    _require(mask_out, "mask_out", torch.uint8, depth)
    if tuple(mask_out.shape) != (B, H, W) or tuple(depth_out.shape) != (B, H, W):
        raise ValueError(f"robot_mask: mask_out / depth_out must have shape {(B, H, W)}")
    if projection_rays.dim() != 3 or tuple(projection_rays.shape[1:]) != (H * W, 3):
        raise ValueError(f"robot_mask: projection_rays must be (B or 1, {H * W}, 3), got {tuple(projection_rays.shape)}")
    pos, quat = camera_position.reshape(-1, 3), camera_quaternion.reshape(-1, 4)
    if pos.shape[0] != quat.shape[0]:
        raise ValueError("robot_mask: camera position and quaternion batches differ")
    if robot_spheres.dim() != 3 or robot_spheres.shape[-1] != 4:
        raise ValueError(f"robot_mask: robot_spheres must be (B or 1, S, 4), got {tuple(robot_spheres.shape)}")
    check(load().curobo_hip_robot_mask(
        ptr(mask_out), ptr(depth_out), ptr(depth), ptr(projection_rays), ptr(pos), ptr(quat), ptr(robot_spheres), B, H, W,
        int(robot_spheres.shape[1]), int(projection_rays.shape[0]), int(pos.shape[0]), int(robot_spheres.shape[0]),
        float(distance_threshold), int(mode), current_stream(depth)))


# ---------------------------------------------------------------------------------------------------- pose refinement
import ctypes as _C  # noqa: E402
from functools import partial  # noqa: E402

POSE_LM_INIT, POSE_LM_UPDATE = 0, 1  # ``mode`` of ``curobo_hip_pose_lm_step``
POSE_WS_ROW = 32                     # CUROBO_HIP_POSE_WS_ROW


def _field_slice(struct, name: str) -> slice:
    """the words of field ``name`` of a ctypes struct of 4-byte words"""
    f = getattr(struct, name)
    return slice(f.offset // 4, (f.offset + f.size) // 4)


def pose_state_field(state: torch.Tensor, struct, name: str) -> torch.Tensor:
    """field ``name`` of a state tensor whose last dimension holds the words of ``struct``: a view, int32 for a scalar c_int32 field"""
    words = state[..., _field_slice(struct, name)]
    return words.view(torch.int32) if dict(struct._fields_)[name] is _C.c_int32 else words


def _ws_bytes(query, *counts: int) -> int:
    nbytes = _C.c_int64(0)
    check(query(*(int(c) for c in counts), _C.cast(_C.pointer(nbytes), _C.c_void_p)))
    return int(nbytes.value)


def _require_workspace(workspace: torch.Tensor, like: torch.Tensor, what: str, where: str = "state's device") -> int:
    if not workspace.is_contiguous() or workspace.device != like.device:
        raise ValueError(f"{what}: workspace must be a contiguous tensor on the {where}")
    return int(workspace.numel() * workspace.element_size())


class PoseLMState(_C.Structure):
    """``curobo_hip_pose_lm_state``: used for its field offsets; the state itself is a device tensor of 4-byte words"""

    _fields_ = [("best_position", _C.c_float * 3), ("best_quaternion", _C.c_float * 4), ("best_error", _C.c_float),
                ("best_sum_sq", _C.c_float), ("best_n_valid", _C.c_int32), ("lambda_damping", _C.c_float),
                ("best_JtJ", _C.c_float * 36), ("best_Jtr", _C.c_float * 6), ("cand_position", _C.c_float * 3),
                ("cand_quaternion", _C.c_float * 4), ("pred_reduction", _C.c_float), ("delta", _C.c_float * 6),
                ("cand_sum_sq", _C.c_float), ("cand_n_valid", _C.c_int32), ("trust_ratio", _C.c_float), ("accepted", _C.c_int32)]


POSE_STATE_WORDS = _C.sizeof(PoseLMState) // 4
POSE_STATE_INT_FIELDS = tuple(n for n, t in PoseLMState._fields_ if t is _C.c_int32)  #: the scalar c_int32 fields; every other word is a float
pose_state_slice = partial(_field_slice, PoseLMState)  #: (name) -> the words of field ``name`` in a state tensor


def pose_sdf_ws_bytes(n_points: int) -> int:
    """``curobo_hip_pose_sdf_ws_bytes``"""
    return _ws_bytes(load().curobo_hip_pose_sdf_ws_bytes, n_points)


def pose_sdf_evaluate(workspace: torch.Tensor, points: torch.Tensor, position: torch.Tensor, quaternion: torch.Tensor, mesh_struct,
                      max_distance: float, distance_threshold: float, use_huber: bool, huber_delta: float,
                      out_distance: Optional[torch.Tensor] = None, out_gradient: Optional[torch.Tensor] = None,
                      out_valid: Optional[torch.Tensor] = None) -> None:
    """``curobo_hip_pose_sdf_evaluate``: points [N, 3] (world frame) against the mesh ``mesh_struct`` (``backends.mesh.Mesh``) at
    the pose ``position`` [3] / ``quaternion`` [4] wxyz on the device -> one row of partial sums per workgroup in ``workspace``
    (uint8 or 4-byte words), and optionally the per-point distance [N], world gradient [N, 3] and valid [N] int32."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"pose_sdf_evaluate: points must be (N, 3), got {tuple(points.shape)}")
    _require(points, "points", torch.float32)
    _require(position, "position", torch.float32, points)
    _require(quaternion, "quaternion", torch.float32, points)
    if position.numel() != 3 or quaternion.numel() != 4:
        raise ValueError("pose_sdf_evaluate: position must hold 3 and quaternion 4 values")
    n = int(points.shape[0])
    for name, t, dt, shape in (("out_distance", out_distance, torch.float32, (n,)), ("out_gradient", out_gradient, torch.float32, (n, 3)),
                               ("out_valid", out_valid, torch.int32, (n,))):
        _require(t, name, dt, points)
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"pose_sdf_evaluate: {name} must have shape {shape}, got {tuple(t.shape)}")
    check(load().curobo_hip_pose_sdf_evaluate(
        ptr(out_distance), ptr(out_gradient), ptr(out_valid), ptr(workspace), _require_workspace(workspace, points, "pose_sdf_evaluate", "points' device"),
        ptr(points), ptr(position), ptr(quaternion), _C.addressof(mesh_struct), float(max_distance), float(distance_threshold),
        int(bool(use_huber)), float(huber_delta), n, current_stream(points)))


def pose_lm_step(state: torch.Tensor, workspace: torch.Tensor, n_points: int, mode: int, lambda_initial: float, lambda_factor: float,
                 lambda_min: float, lambda_max: float, rho_min: float, minimum_valid_count: int = 10) -> None:
    """``curobo_hip_pose_lm_step`` on ``state`` (float32 [POSE_STATE_WORDS], the layout of ``PoseLMState``)"""
    _require(state, "state", torch.float32)
    if state.numel() != POSE_STATE_WORDS:
        raise ValueError(f"pose_lm_step: state must hold {POSE_STATE_WORDS} words, got {state.numel()}")
    check(load().curobo_hip_pose_lm_step(
        ptr(state), ptr(workspace), _require_workspace(workspace, state, "pose_lm_step"), int(n_points), int(mode), float(lambda_initial),
        float(lambda_factor), float(lambda_min), float(lambda_max), float(rho_min), int(minimum_valid_count), current_stream(state)))


# ---------------------------------------------------------------------------------------------------- point-to-plane ICP
POSE_ICP_COARSE, POSE_ICP_FINE, POSE_ICP_FINALIZE = 0, 1, 2  # ``mode`` of ``curobo_hip_pose_icp_step``


class PoseICPState(_C.Structure):
    """``curobo_hip_pose_icp_state``: used for its field offsets; the states are a device tensor [H, POSE_ICP_STATE_WORDS]"""

    _fields_ = [("T", _C.c_float * 12), ("error", _C.c_float), ("iterations", _C.c_int32), ("stopped", _C.c_int32),
                ("solver_failed", _C.c_int32), ("n_valid", _C.c_int32), ("x", _C.c_float * 6), ("reserved", _C.c_int32)]


POSE_ICP_STATE_WORDS = _C.sizeof(PoseICPState) // 4
POSE_ICP_STATE_INT_FIELDS = tuple(n for n, t in PoseICPState._fields_ if t is _C.c_int32)  #: the scalar c_int32 fields; every other word is a float
pose_icp_state_slice = partial(_field_slice, PoseICPState)  #: (name) -> the words of field ``name`` in each row of a state tensor


def pose_icp_ws_bytes(n_hypotheses: int, n_mesh: int) -> int:
    """``curobo_hip_pose_icp_ws_bytes``"""
    return _ws_bytes(load().curobo_hip_pose_icp_ws_bytes, n_hypotheses, n_mesh)


def _require_icp_state(state: torch.Tensor, what: str) -> int:
    _require(state, "state", torch.float32)
    if state.dim() != 2 or state.shape[1] != POSE_ICP_STATE_WORDS:
        raise ValueError(f"{what}: state must be (H, {POSE_ICP_STATE_WORDS}), got {tuple(state.shape)}")
    return int(state.shape[0])


def pose_icp_correspond(workspace: torch.Tensor, mesh_points: torch.Tensor, mesh_normals: torch.Tensor, observed_points: torch.Tensor,
                        state: torch.Tensor, distance_threshold: float, use_huber: bool, huber_delta: float, honour_stopped: bool = True,
                        out_index: Optional[torch.Tensor] = None, out_distance: Optional[torch.Tensor] = None) -> None:
    """``curobo_hip_pose_icp_correspond``: mesh_points / mesh_normals [M, 3] at the H poses of ``state`` [H, POSE_ICP_STATE_WORDS]
    against observed_points [O, 3] -> per hypothesis one row of partial sums per 64 samples in ``workspace``, and optionally
    the per-sample nearest index [H, M] int32 (-1 when invalid) and distance [H, M]."""
    what = "pose_icp_correspond"
    h = _require_icp_state(state, what)
    for name, t in (("mesh_points", mesh_points), ("mesh_normals", mesh_normals), ("observed_points", observed_points)):
        _require(t, name, torch.float32, state)
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be (N, 3), got {tuple(t.shape)}")
    m, o = int(mesh_points.shape[0]), int(observed_points.shape[0])
    if tuple(mesh_normals.shape) != (m, 3):
        raise ValueError(f"{what}: mesh_normals must have shape {(m, 3)}, got {tuple(mesh_normals.shape)}")
    for name, t, dt in (("out_index", out_index, torch.int32), ("out_distance", out_distance, torch.float32)):
        _require(t, name, dt, state)
        if t is not None and tuple(t.shape) != (h, m):
            raise ValueError(f"{what}: {name} must have shape {(h, m)}, got {tuple(t.shape)}")
    check(load().curobo_hip_pose_icp_correspond(
        ptr(out_index), ptr(out_distance), ptr(workspace), _require_workspace(workspace, state, what), ptr(mesh_points), ptr(mesh_normals),
        ptr(observed_points), ptr(state), float(distance_threshold), int(bool(use_huber)), float(huber_delta), int(bool(honour_stopped)),
        h, m, o, current_stream(state)))


def pose_icp_step(state: torch.Tensor, workspace: torch.Tensor, n_mesh: int, mode: int) -> None:
    """``curobo_hip_pose_icp_step`` on ``state`` [H, POSE_ICP_STATE_WORDS] (rows in the layout of ``PoseICPState``)"""
    what = "pose_icp_step"
    h = _require_icp_state(state, what)
    check(load().curobo_hip_pose_icp_step(ptr(state), ptr(workspace), _require_workspace(workspace, state, what), h, int(n_mesh), int(mode),
                                          current_stream(state)))


def pose_icp_select(out_index: torch.Tensor, state: torch.Tensor, out_error: Optional[torch.Tensor] = None,
                    out_transform: Optional[torch.Tensor] = None) -> None:
    """``curobo_hip_pose_icp_select``: out_index [1] int32 = the lowest-index minimum of the H errors; optionally its error [1]
    and its T [12]"""
    what = "pose_icp_select"
    h = _require_icp_state(state, what)
    for name, t, dt, n in (("out_index", out_index, torch.int32, 1), ("out_error", out_error, torch.float32, 1),
                           ("out_transform", out_transform, torch.float32, 12)):
        _require(t, name, dt, state)
        if t is not None and t.numel() != n:
            raise ValueError(f"{what}: {name} must hold {n} values, got {t.numel()}")
    if out_index is None:
        raise ValueError(f"{what}: out_index must not be None")
    check(load().curobo_hip_pose_icp_select(ptr(out_index), ptr(out_error), ptr(out_transform), ptr(state), h, current_stream(state)))
