"""HIP backend of the PRM graph planner (``csrc/graph_planner.hip``: graph_steer_kernel
and graph_knn_kernel).  Same conventions as the other backends:
pre-allocated tensors in, mutated in place, current stream."""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._lib import Scene, check, current_stream, load, ptr


def graph_steer(out_node: Optional[torch.Tensor], out_index: Optional[torch.Tensor], out_feasible: Optional[torch.Tensor],
                max_steps_ws: Optional[torch.Tensor], start: torch.Tensor, target: Optional[torch.Tensor],
                cspace_distance_weight: Optional[torch.Tensor], cspace_similarity_threshold: float, point_mode: bool,
                kin, scene: Optional[Scene]) -> None:
    """Steer the edges start[n, ld] -> target[n, ld] until infeasible (``curobo_hip_graph_steer``): out_node[n, dof + 1],
    out_index[n] (int32), max_steps_ws[1] (int32, device workspace); ``point_mode``: out_feasible[n] (uint8) of the start
    rows.  ``kin``: the robot's ``KinematicsParams`` (a single sphere set)."""
    n, ld = int(start.shape[0]), int(start.stride(0))
    if start.stride(1) != 1 or (target is not None and tuple(target.stride()) != tuple(start.stride())):
        raise ValueError("graph_steer: start / target rows must be contiguous with equal strides")
    sc = kin.self_collision
    pairs = None if sc is None or sc.collision_pairs is None or sc.collision_pairs.numel() == 0 else sc.collision_pairs
    check(load().curobo_hip_graph_steer(
        ptr(out_node), ptr(out_index), ptr(out_feasible), ptr(max_steps_ws), ptr(start), ptr(target), ld,
        ptr(cspace_distance_weight), float(cspace_similarity_threshold), n, int(bool(point_mode)),
        ptr(kin.joint_limits_position), ptr(kin.fixed_transforms), ptr(kin.link_spheres), ptr(kin.joint_map_type),
        ptr(kin.joint_map), ptr(kin.link_map), ptr(kin.link_sphere_idx_map), ptr(kin.link_chain_data),
        ptr(kin.link_chain_offsets), ptr(kin.joint_offset_map), ptr(sc.sphere_padding), ptr(pairs),
        None if scene is None else C.addressof(scene), int(kin.num_dof), int(kin.fixed_transforms.shape[0]),
        int(kin.link_sphere_idx_map.shape[0]), 0 if pairs is None else int(pairs.shape[0]), int(kin.link_chain_data.shape[0]),
        current_stream(start)))


def graph_knn(out_idx: torch.Tensor, queries: torch.Tensor, nodes: torch.Tensor, cspace_distance_weight: torch.Tensor,
              n_nodes: int, dof: int, k: int) -> None:
    """out_idx[q, k] (int32): the k nearest of the first ``n_nodes`` rows of nodes to each query row under the weighted
    distance, nearest first, ties to the lower index (``curobo_hip_graph_knn``)."""
    for t in (queries, nodes):
        if t.stride(1) != 1:
            raise ValueError("graph_knn: rows must be contiguous")
    check(load().curobo_hip_graph_knn(
        ptr(out_idx), ptr(queries), int(queries.stride(0)), ptr(nodes), int(nodes.stride(0)), ptr(cspace_distance_weight),
        int(queries.shape[0]), int(n_nodes), int(dof), int(k), current_stream(out_idx)))
