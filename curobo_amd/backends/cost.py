"""HIP backend for the tool-pose and c-space POSITION cost kernels, and for the support-polygon cost (torch code in the
reference: ``geom/convex_polygon_helper.py``, ``cost/cost_support_polygon.py``).

The reference runs these through NVIDIA Warp without a backend hook
(``curobo/_src/cost/wp_tool_pose.py:698-914``, ``cost/wp_cspace_position.py:232-362``); the
functions keep the reference backends' style: pre-allocated tensors in, mutated in place, launched
on the current stream.  Argument order = the Warp kernels' input order.
"""

from __future__ import annotations

from typing import Optional

import torch

from .._lib import check, current_stream, load, ptr


def tool_pose_distance(
    out_distance: torch.Tensor,
    out_position_distance: torch.Tensor,
    out_rotation_distance: torch.Tensor,
    out_position_gradient: torch.Tensor,
    out_rotation_gradient: torch.Tensor,
    out_goalset_idx: torch.Tensor,
    current_position: torch.Tensor,
    current_quat: torch.Tensor,
    goal_position: torch.Tensor,
    goal_quat: torch.Tensor,
    idxs_goal: torch.Tensor,
    position_orientation_weight: torch.Tensor,
    terminal_pose_axes_weight_factor: torch.Tensor,
    non_terminal_pose_axes_weight_factor: torch.Tensor,
    terminal_pose_convergence_tolerance: torch.Tensor,
    non_terminal_pose_convergence_tolerance: torch.Tensor,
    project_distance_to_goal: torch.Tensor,
    batch_size: int,
    horizon: int,
    num_links: int,
    num_goalset: int,
    rotation_method: int = 0,
):
    check(load().curobo_hip_tool_pose_distance(
        ptr(out_distance), ptr(out_position_distance), ptr(out_rotation_distance), ptr(out_position_gradient),
        ptr(out_rotation_gradient), ptr(out_goalset_idx), ptr(current_position), ptr(current_quat),
        ptr(goal_position), ptr(goal_quat), ptr(idxs_goal), ptr(position_orientation_weight),
        ptr(terminal_pose_axes_weight_factor), ptr(non_terminal_pose_axes_weight_factor),
        ptr(terminal_pose_convergence_tolerance), ptr(non_terminal_pose_convergence_tolerance),
        ptr(project_distance_to_goal), batch_size, horizon, num_links, num_goalset, rotation_method,
        current_stream(out_distance),
    ))


def cspace_position_cost(
    out_cost: torch.Tensor,
    out_grad_p: torch.Tensor,
    out_grad_tau: Optional[torch.Tensor],
    pos: torch.Tensor,
    effort: Optional[torch.Tensor],
    cspace_target: torch.Tensor,
    cspace_target_idx: torch.Tensor,
    p_b: torch.Tensor,
    effort_b: torch.Tensor,
    weight: torch.Tensor,
    activation_distance: torch.Tensor,
    cspace_target_weight: torch.Tensor,
    cspace_target_dof_weight: torch.Tensor,
    squared_l2_reg_weight: torch.Tensor,
    current_position: torch.Tensor,
    current_velocity: torch.Tensor,
    idxs_current_state: torch.Tensor,
    v_b: torch.Tensor,
    state_dt: torch.Tensor,
    write_grad: bool,
    batch_size: int,
    horizon: int,
    dof: int,
):
    check(load().curobo_hip_cspace_position_cost(
        ptr(out_cost), ptr(out_grad_p), ptr(out_grad_tau), ptr(pos), ptr(effort), ptr(cspace_target),
        ptr(cspace_target_idx), ptr(p_b), ptr(effort_b), ptr(weight), ptr(activation_distance),
        ptr(cspace_target_weight), ptr(cspace_target_dof_weight), ptr(squared_l2_reg_weight),
        ptr(current_position), ptr(current_velocity), ptr(idxs_current_state), ptr(v_b), ptr(state_dt),
        int(write_grad), batch_size, horizon, dof, current_stream(out_cost),
    ))


def rollout_point_aggregate(
    out_cost: torch.Tensor,
    grad_q: Optional[torch.Tensor],
    pose_cost: Optional[torch.Tensor],
    cspace_cost: Optional[torch.Tensor],
    cspace_grad: Optional[torch.Tensor],
    self_cost: Optional[torch.Tensor],
    scene_cost: Optional[torch.Tensor],
    rows: int,
    num_links: int,
    dof: int,
    num_spheres: int,
):
    """out_cost[r] = all cost terms of rollout row r summed; grad_q[r] += cspace_grad[r]."""
    check(load().curobo_hip_rollout_point_aggregate(
        ptr(out_cost), ptr(grad_q), ptr(pose_cost), ptr(cspace_cost), ptr(cspace_grad), ptr(self_cost),
        ptr(scene_cost), rows, num_links, dof, num_spheres, current_stream(out_cost),
    ))


def rollout_point_aggregate_terms(out_cost, grad_q, pose_cost, cspace_cost, cspace_grad, self_cost, scene_cost, extra_cost,
                                  rows: int, num_links: int, dof: int, num_spheres: int):
    """``rollout_point_aggregate`` with one more per-row term: out_cost[r] also takes extra_cost[r] (None = none)."""
    check(load().curobo_hip_rollout_point_aggregate_terms(
        ptr(out_cost), ptr(grad_q), ptr(pose_cost), ptr(cspace_cost), ptr(cspace_grad), ptr(self_cost),
        ptr(scene_cost), ptr(extra_cost), rows, num_links, dof, num_spheres, current_stream(out_cost),
    ))


def _f32(name: str, t: torch.Tensor, *shape) -> None:
    """a contiguous float32 tensor of ``shape`` (None = any extent)"""
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous torch.float32 tensor, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, t.shape)):
        want = "(" + ", ".join("*" if s is None else str(s) for s in shape) + ")"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")


def _i32(name: str, t: torch.Tensor, n: int) -> None:
    if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise ValueError(f"{name} must be a contiguous torch.int32 tensor of shape ({n},), got {t.dtype} {tuple(t.shape)}")


def convex_hull_2d(out_hulls: torch.Tensor, out_counts: torch.Tensor, points: torch.Tensor, padding: float = 0.0):
    """points [N, n_pts, 2] -> out_hulls [N, n_pts, 2], out_counts [N] int32 (reference ``_compute_convex_hull_single`` per set,
    ``geom/convex_polygon_helper.py:106-216``): counter-clockwise from the lowest vertex, padded, rows past the count repeat
    the last vertex.  ``3 <= n_pts <= 64``."""
    _f32("points", points, None, None, 2)
    N, n_pts = int(points.shape[0]), int(points.shape[1])
    if not 3 <= n_pts <= 64:  # (the launcher's own check, made before the stream is asked for)
        raise ValueError(f"convex_hull_2d: n_pts must be in 3..64, got {n_pts}")
    _f32("out_hulls", out_hulls, N, n_pts, 2)
    _i32("out_counts", out_counts, N)
    check(load().curobo_hip_convex_hull_2d(ptr(out_hulls), ptr(out_counts), ptr(points), float(padding), N, n_pts,
                                           current_stream(out_hulls)))


def support_polygon_cost(out_cost: torch.Tensor, out_grad_com: torch.Tensor, out_signed_distance: Optional[torch.Tensor],
                         com: torch.Tensor, hulls: torch.Tensor, counts: Optional[torch.Tensor], idxs_hull: torch.Tensor,
                         weight: torch.Tensor, inside_cost_weight: float, margin_target: float = 0.1,
                         smoothing: float = 0.01, cost_mode: int = 0):
    """com [B, H, 4] against hull ``idxs_hull[b]`` of hulls [N, M, 2] -> out_cost [B, H], out_grad_com [B, H, 4] (weight
    applied, xy only) and out_signed_distance [B, H] or None (reference ``compute_point_hull_distance`` +
    ``_compute_support_polygon_cost_vectorized``).  ``counts`` None: every row of a hull forms an edge (the reference's
    padded tensor); else hull i has ``counts[i]`` vertices.  ``cost_mode`` 1: the cost is ``weight * signed distance`` itself.
    ``M <= 32``."""
    _f32("com", com, None, None, 4)
    B, H = int(com.shape[0]), int(com.shape[1])
    _f32("hulls", hulls, None, None, 2)
    N, M = int(hulls.shape[0]), int(hulls.shape[1])
    if not 1 <= M <= 32:
        raise ValueError(f"support_polygon_cost: max_vertices must be in 1..32, got {M}")
    _f32("out_cost", out_cost, B, H)
    _f32("out_grad_com", out_grad_com, B, H, 4)
    if out_signed_distance is not None:
        _f32("out_signed_distance", out_signed_distance, B, H)
    if counts is not None:
        _i32("counts", counts, N)
    _i32("idxs_hull", idxs_hull, B)
    _f32("weight", weight, 1)
    check(load().curobo_hip_support_polygon_cost(
        ptr(out_cost), ptr(out_grad_com), ptr(out_signed_distance), ptr(com), ptr(hulls), ptr(counts), ptr(idxs_hull),
        ptr(weight), float(inside_cost_weight), float(margin_target), float(smoothing), B, H, N, M, int(cost_mode),
        current_stream(out_cost)))


def cspace_state_cost(
    out_cost, out_grad_p, out_grad_v, out_grad_a, out_grad_j, out_grad_tau, pos, vel, acc, jerk, effort, state_dt,
    target_joint_position, idxs_target_joint_position, p_b, v_b, a_b, j_b, effort_b, weight, activation_distance,
    squared_l2_regularization_weights, cspace_target_weight, cspace_non_terminal_weight_factor,
    cspace_target_dof_weight, write_grad: bool, batch_size: int, horizon: int, dof: int,
    retime_weights: bool = False, retime_regularization_weights: bool = False,
):
    """reference ``forward_cspace_state_warp`` (``cost/wp_cspace_state.py:20-287``), argument order =
    the Warp kernel's inputs then outputs-first like the other backends."""
    check(load().curobo_hip_cspace_state_cost(
        ptr(out_cost), ptr(out_grad_p), ptr(out_grad_v), ptr(out_grad_a), ptr(out_grad_j), ptr(out_grad_tau), ptr(pos),
        ptr(vel), ptr(acc), ptr(jerk), ptr(effort), ptr(state_dt), ptr(target_joint_position),
        ptr(idxs_target_joint_position), ptr(p_b), ptr(v_b), ptr(a_b), ptr(j_b), ptr(effort_b), ptr(weight),
        ptr(activation_distance), ptr(squared_l2_regularization_weights), ptr(cspace_target_weight),
        ptr(cspace_non_terminal_weight_factor), ptr(cspace_target_dof_weight), int(write_grad), batch_size, horizon, dof,
        int(retime_weights), int(retime_regularization_weights), current_stream(out_cost),
    ))


def cspace_l2_distance(out_cost, out_grad_p, pos, target, target_idx, weight, terminal_dof_weight,
                       non_terminal_dof_weight, write_grad: bool, batch_size: int, horizon: int, dof: int):
    """reference ``forward_l2_warp`` (``cost/wp_torch_cspace_dist.py:12-78``; outputs first)."""
    check(load().curobo_hip_cspace_l2_distance(
        ptr(out_cost), ptr(out_grad_p), ptr(pos), ptr(target), ptr(target_idx), ptr(weight), ptr(terminal_dof_weight),
        ptr(non_terminal_dof_weight), int(write_grad), batch_size, horizon, dof, current_stream(out_cost),
    ))
