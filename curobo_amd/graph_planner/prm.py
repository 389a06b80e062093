"""PRM graph planner (reference ``curobo/_src/graph_planner/``: ``graph_planner_prm.py``, ``graph/*``,
``search/*``).  A roadmap of collision-free configurations joined by collision-free straight edges, grown
around the start-goal line until every query has a path, then shortcut-pruned.

The two hot loops are HIP (``backends/graph.py``): edge steering with per-point feasibility
(``curobo_hip_graph_steer``, which also answers "is each of these configurations feasible") and the weighted
k-nearest-neighbour search (``curobo_hip_graph_knn``).  Node bookkeeping, the grow loop and the shortest-path
search (Dijkstra, ``graph.RoadmapGraph``) stay on the host.  Single environment only, as in the reference.
"""

from __future__ import annotations

import math
import random
import time
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from .graph import RoadmapGraph


@dataclass
class PRMGraphPlannerCfg:
    """reference ``PRMGraphPlannerCfg`` (graph_planner_prm_cfg.py); the defaults are
    ``content/configs/task/graph_planner/exact_graph_planner.yml``"""

    max_nodes: int = 20000
    steer_buffer_size: int = 5000
    cspace_similarity_threshold: float = 0.005
    sample_rejection_ratio: int = 10
    neighbors_per_node: int = 10
    feasibility_buffer_size: int = 2000
    new_nodes_per_iteration: int = 20
    max_path_finding_iterations: int = 10
    min_finetune_iterations: int = 2
    use_default_position_heuristic: bool = True
    exploration_radius: float = 1.05
    exploration_radius_growth_factor: float = 1.05
    sampler_seed: int = 0
    sampler_buffer_size: int = 2000
    connect_terminal_nodes_with_nearest: bool = False
    ellipsoid_projection_method: str = "householder"
    neighbors_per_node_growth_factor: float = 1.05
    new_nodes_per_iteration_growth_factor: float = 1.05
    #: per-joint weight of the c-space distance (the reference's planner uses ones)
    cspace_distance_weight: Optional[List[float]] = None
    #: seed of the host choice of which unsolved query grows the roadmap next
    graph_path_finder_seed: int = 0

    @staticmethod
    def yaml_keys() -> List[str]:
        return [f for f in PRMGraphPlannerCfg.__dataclass_fields__ if f not in ("cspace_distance_weight", "graph_path_finder_seed")]


@dataclass
class GraphPlannerResult:
    """reference ``GraphPlannerResult`` (graph_planner/result.py)"""

    success: torch.Tensor
    path_length: Optional[torch.Tensor] = None
    plan_waypoints: Optional[List[Optional[torch.Tensor]]] = None
    interpolated_waypoints: Optional[torch.Tensor] = None
    solve_time: float = 0.0
    valid_query: bool = True
    debug_info: Optional[str] = None
    joint_names: Optional[List[str]] = None


#: largest k of the k-nearest-neighbour launch (curobo_hip_graph_knn)
KNN_MAX_K = 64


def _cdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """pairwise Euclidean distances computed from the differences: the matrix-product expansion torch.cdist switches to
    above 25 rows loses ~1e-3 at joint values of a few radians, which would blur the exact (0) and 0.005 node merges"""
    return torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist")


# ---------------------------------------------------------------------------------------------- steering rules
def steer_num_steps(start: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, threshold: float) -> torch.Tensor:
    """num_steps per edge = ceil(max_k |w_k (t_k - s_k)| / threshold) + 1 (connector_linear.py:132-136)"""
    return torch.ceil(((target - start) * weight).abs().max(dim=-1).values / threshold) + 1


def steer_points(start: torch.Tensor, target: torch.Tensor, max_steps: int) -> torch.Tensor:
    """[E, max_steps + 1, D]: every edge at the batch-wide step count, coefficient k / max_steps (connector_linear.py:138-147)"""
    coeff = torch.arange(max_steps + 1, device=start.device, dtype=start.dtype) / max_steps
    return start.unsqueeze(1) + coeff.view(1, -1, 1) * (target - start).unsqueeze(1)


def last_feasible_index(mask: torch.Tensor) -> torch.Tensor:
    """mask [E, h] (True = feasible) -> [E]: the point before the first infeasible one, clamped to 0; the end point when
    none is infeasible (connector_linear.py:151-180)"""
    h = mask.shape[1]
    k = torch.arange(h, device=mask.device).view(1, h)
    first = torch.where(~mask, k, torch.full_like(k, h)).min(dim=1).values
    return torch.where(first < h, first - 1, torch.full_like(first, h - 1)).clamp(min=0)


def transform_unit_ball_to_ellipsoid_householder(x_start, x_goal, weight, max_sampling_radius, unit_ball, low, high,
                                                 clamp: bool = True) -> torch.Tensor:
    """unit-ball samples [n, D] -> the ellipsoid whose major axis runs along start -> goal (node_sampling_strategy.py:
    163-330, Householder form): the reflection H = I - 2 v v^T maps e1 onto the weighted start-goal direction; semi-axes
    c_max / 2 along it and (c_max^2 - c_min^2) / 2 across, c_min = the weighted start-goal distance (the reference's
    scaling, kept as written); the samples are then unweighted, centred and clamped to the joint limits"""
    direction = x_goal - x_start
    c_min = torch.norm(direction * weight)
    direction = direction / c_min
    e1 = torch.zeros_like(direction)
    e1[0] = 1.0
    v = direction - e1 if bool(direction[0] >= 0) else direction + e1
    vn = torch.norm(v)
    v = v / vn if float(vn) > 1e-10 else torch.zeros_like(direction)
    C = torch.eye(direction.shape[0], device=direction.device, dtype=direction.dtype) - 2.0 * torch.outer(v, v)
    scale = torch.empty_like(x_start)
    scale[0:1] = max_sampling_radius / 2.0
    scale[1:] = (max_sampling_radius ** 2 - c_min ** 2) / 2.0
    x = ((C @ torch.diag(scale)) @ unit_ball.T).T / weight + (x_start + x_goal) / 2.0
    return torch.clamp(x, low, high).contiguous() if clamp else x


# ---------------------------------------------------------------------------------------------- feasibility
class GraphFeasibility:
    """Edge steering and point feasibility against a ``RobotCollisionChecker``'s robot and world: the fused HIP launch
    for scenes of cuboids, analytic primitives and voxel grids; for scenes with meshes, or robots whose 16 configurations
    do not fit in LDS, the materialised path (the points interpolated explicitly, then ``checker.validate`` in chunks of
    ``feasibility_buffer_size``)."""

    def __init__(self, checker, threshold: float, weight: torch.Tensor, buffer_size: int):
        self.checker, self.threshold, self.weight, self.buffer_size = checker, float(threshold), weight, int(buffer_size)
        self._ws = torch.zeros(1, dtype=torch.int32, device=weight.device)

    @property
    def kin(self):
        return self.checker.kinematics.kinematics_config

    def uses_fused(self) -> bool:
        """the fused launch covers the scene (no meshes) and 16 of the robot's configurations fit in LDS"""
        from ..backends import rollout as rollout_hip
        from ..rollout.base import obstacle_slots, scene_has_meshes

        s = self.checker.scene
        if scene_has_meshes(s) or getattr(s, "meshes", None) is not None:
            return False
        k = self.kin
        sc = k.self_collision
        pairs = 0 if sc is None or sc.collision_pairs is None else int(sc.collision_pairs.shape[0])
        L, S = int(k.fixed_transforms.shape[0]), int(k.link_sphere_idx_map.shape[0])
        need = rollout_hip.rollout_ik_fused_lds_bytes(k.num_dof, L, S, pairs, int(k.link_chain_data.shape[0]), obstacle_slots(s))
        return need <= rollout_hip.FUSED_LDS_LIMIT - 64 and k.num_dof <= 64 and L <= 128 and S < 4096

    def _struct(self):
        return None if self.checker.scene is None else self.checker.scene.struct

    def validate_materialised(self, q: torch.Tensor) -> torch.Tensor:
        """q [N, D] -> bool [N] through ``checker.validate`` in chunks"""
        out = [self.checker.validate(q[i:i + self.buffer_size].unsqueeze(1)).view(-1) for i in range(0, q.shape[0], self.buffer_size)]
        return torch.cat(out) if out else torch.zeros(0, dtype=torch.bool, device=q.device)

    def feasible(self, q: torch.Tensor) -> torch.Tensor:
        q = q.contiguous().float()
        if not self.uses_fused():
            return self.validate_materialised(q)
        from ..backends import graph as graph_hip

        out = torch.empty(q.shape[0], dtype=torch.uint8, device=q.device)
        graph_hip.graph_steer(None, None, out, None, q, None, None, self.threshold, True, self.kin, self._struct())
        return out.bool()

    def steer(self, start: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """start, target [E, >= D] -> (last feasible nodes [E, D + 1] (index column 0), their step index [E])"""
        D = self.weight.shape[0]
        E = start.shape[0]
        s, t = start[:, :D].contiguous().float(), target[:, :D].contiguous().float()
        if not self.uses_fused():
            ms = int(steer_num_steps(s, t, self.weight, self.threshold).max().item())
            pts = steer_points(s, t, ms)
            idx = last_feasible_index(self.validate_materialised(pts.reshape(-1, D)).view(E, ms + 1))
            node = torch.cat([pts[torch.arange(E, device=s.device), idx], torch.zeros(E, 1, device=s.device)], 1)
            return node, idx.to(torch.int32)
        from ..backends import graph as graph_hip

        node = torch.empty(E, D + 1, device=s.device)
        idx = torch.empty(E, dtype=torch.int32, device=s.device)
        graph_hip.graph_steer(node, idx, None, self._ws, s, t, self.weight, self.threshold, False, self.kin, self._struct())
        return node, idx


# ---------------------------------------------------------------------------------------------- planner
class PRMGraphPlanner:
    """reference ``PRMGraphPlanner`` (graph_planner_prm.py) over a ``RobotCollisionChecker`` (robot + world, activation
    distance 0).  ``default_joint_position`` [D]: the default-configuration heuristic's node."""

    def __init__(self, config: PRMGraphPlannerCfg, checker, default_joint_position: Optional[torch.Tensor] = None,
                 joint_names: Optional[List[str]] = None):
        from ..solver.seed_ik import HaltonSeeds

        self.config = config
        self.checker = checker
        k = checker.kinematics.kinematics_config
        if int(getattr(k, "num_envs", 1)) > 1:
            raise ValueError("the graph planner plans in a single environment (one sphere set)")
        self.device = k.joint_limits_position.device
        self.action_dim = D = int(k.num_dof)
        self.joint_names = joint_names
        self.low, self.high = k.joint_limits_position[0].contiguous(), k.joint_limits_position[1].contiguous()
        w = config.cspace_distance_weight
        self.cspace_distance_weight = (torch.ones(D, device=self.device) if w is None else
                                       torch.as_tensor(w, dtype=torch.float32, device=self.device).contiguous())
        self.feasibility = GraphFeasibility(checker, config.cspace_similarity_threshold, self.cspace_distance_weight,
                                            config.feasibility_buffer_size)
        self.sampler = HaltonSeeds(D, self.low, self.high, seed=config.sampler_seed, store_buffer=config.sampler_buffer_size)
        self.graph = RoadmapGraph()
        self._nodes = torch.zeros(config.max_nodes, D + 1, device=self.device)
        self._n = 0
        self._rng = random.Random(config.graph_path_finder_seed)
        self.default_joint_position = None if default_joint_position is None else \
            torch.as_tensor(default_joint_position, dtype=torch.float32, device=self.device).view(D)
        self._default_feasible = None
        self._default_node = None

    # ---- node buffer (graph/node_manager.py)
    @property
    def n_nodes(self) -> int:
        return self._n

    @property
    def valid_node_buffer(self) -> torch.Tensor:
        return self._nodes[:self._n]

    def weighted_distance(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return torch.norm((b - a) * self.cspace_distance_weight, dim=-1)

    def reset_buffer(self) -> None:
        """empty roadmap (reference ``reset_buffer``)"""
        self.graph.reset()
        self._nodes.zero_()
        self._n = 0
        self._default_feasible = None
        self._default_node = None

    def reset_seed(self) -> None:
        self.sampler.reset()
        self._rng = random.Random(self.config.graph_path_finder_seed)

    def reset_graph(self) -> None:
        self.reset_buffer()

    def _append(self, nodes: torch.Tensor) -> torch.Tensor:
        n = nodes.shape[0]
        if self._n + n >= self._nodes.shape[0]:
            raise RuntimeError(f"reached max_nodes={self._nodes.shape[0]} in the roadmap ({self._n} used, {n} more); "
                               "reduce the planning attempts or raise max_nodes")
        D = self.action_dim
        self._nodes[self._n:self._n + n, :D] = nodes
        self._nodes[self._n:self._n + n, D] = torch.arange(self._n, self._n + n, device=self.device, dtype=torch.float32)
        out = self._nodes[self._n:self._n + n]
        self._n += n
        return out

    def _unique(self, nodes: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """(representatives, inverse): each node maps to the first node within ``threshold`` of it (node_distance.py
        jit_get_unique_nodes)"""
        d = _cdist(nodes * self.cspace_distance_weight, nodes * self.cspace_distance_weight)
        close = d <= threshold
        close |= torch.eye(nodes.shape[0], dtype=torch.bool, device=nodes.device)
        first = close.int().argmax(dim=1)
        uniq, inv = torch.unique(first, return_inverse=True)
        return nodes[uniq], inv

    def add_nodes_to_roadmap(self, nodes: torch.Tensor, add_exact_node: bool = False) -> torch.Tensor:
        """nodes [B, D] -> [B, D + 1]: each matched to a roadmap node within the similarity threshold (exactly equal with
        ``add_exact_node``), appended otherwise"""
        D = self.action_dim
        thr = 0.0 if add_exact_node else self.config.cspace_similarity_threshold
        if self._n == 0:
            uniq, inv = self._unique(nodes, thr)
            return self._append(uniq)[inv]
        uniq, inv = self._unique(nodes, thr)
        dist = _cdist(uniq * self.cspace_distance_weight, self.valid_node_buffer[:, :D] * self.cspace_distance_weight)
        dmin, closest = dist.min(dim=-1)
        exists = dmin <= thr
        out = torch.cat([uniq, torch.zeros(uniq.shape[0], 1, device=self.device)], 1)
        out[exists, D] = closest[exists].float()
        if bool((~exists).any()):
            new = self._append(uniq[~exists])
            out[~exists, D] = new[:, D]
        return out[inv]

    def get_nodes_in_path(self, paths: List[Optional[List[int]]]) -> List[Optional[torch.Tensor]]:
        return [None if p is None else self._nodes[p, :self.action_dim] for p in paths]

    # ---- roadmap construction (graph/constructor.py)
    def steer_and_register_edges(self, start_nodes: torch.Tensor, goal_nodes: torch.Tensor, add_exact_node: bool = False) -> None:
        D = self.action_dim
        steered, _ = self.feasibility.steer(start_nodes, goal_nodes)
        in_map = self.add_nodes_to_roadmap(steered[:, :D], add_exact_node)
        dist = self.weighted_distance(start_nodes[:, :D], in_map[:, :D]).tolist()
        si = start_nodes[:, D].to(torch.int64).tolist()
        gi = in_map[:, D].to(torch.int64).tolist()
        self.graph.add_edges(zip(si, gi, dist))

    def find_nearest_neighbors(self, queries: torch.Tensor, k: int) -> torch.Tensor:
        """[B, D + 1] roadmap nodes nearest to each query, [B, k, D + 1]"""
        from ..backends import graph as graph_hip

        k = min(int(k), self._n, KNN_MAX_K)  # (neighbors_per_node grows x1.05 per iteration: capped at the launch's limit)
        idx = torch.empty(queries.shape[0], k, dtype=torch.int32, device=self.device)
        graph_hip.graph_knn(idx, queries[:, :self.action_dim].contiguous().float(), self.valid_node_buffer, self.cspace_distance_weight,
                            self._n, self.action_dim, k)
        return self._nodes[idx.long()]

    def connect_nodes(self, new_nodes: torch.Tensor, neighbors_per_node: int = 10, add_exact_node: bool = False) -> None:
        if new_nodes.shape[0] == 0:
            return
        D = self.action_dim
        if new_nodes.shape[-1] != D + 1:
            new_nodes = torch.cat([new_nodes, torch.zeros(new_nodes.shape[0], 1, device=self.device)], 1)
        near = self.find_nearest_neighbors(new_nodes, neighbors_per_node)
        kk = near.shape[1]
        goal = new_nodes.unsqueeze(1).expand(-1, kk, -1).reshape(-1, D + 1)
        self.steer_and_register_edges(near.reshape(-1, D + 1), goal, add_exact_node)

    def _default_node_in_roadmap(self):
        if self.config.use_default_position_heuristic and self._default_feasible is None and self.default_joint_position is not None:
            q = self.default_joint_position.view(1, -1)
            self._default_feasible = bool(self.feasibility.feasible(q).item())
            if self._default_feasible:
                self._default_node = self.add_nodes_to_roadmap(q.clone(), add_exact_node=True)
        return self._default_node if self._default_feasible else None

    def initialize_terminal_graph_connections(self, x_start: torch.Tensor, x_goal: torch.Tensor):
        B = x_start.shape[0]
        self._default_node_in_roadmap()
        both = self.add_nodes_to_roadmap(torch.cat([x_start, x_goal], 0), add_exact_node=True).view(2, B, -1)
        s, g = both[0], both[1]
        ss, gs = torch.cat([s, g], 0), torch.cat([g, s], 0)
        dn = self._default_node if (self.config.use_default_position_heuristic and self._default_feasible) else None
        if dn is not None:
            dr = dn.view(1, -1).expand(B, -1)
            ss = torch.cat([ss, s, dr, g, dr], 0)
            gs = torch.cat([gs, dr, s, dr, g], 0)
        self.steer_and_register_edges(ss, gs, add_exact_node=False)
        if self.config.connect_terminal_nodes_with_nearest:
            self.connect_nodes(torch.cat([x_start, x_goal], 0), self.config.neighbors_per_node)
        return s, g

    # ---- sampling (graph/node_sampling_strategy.py)
    def _unit_ball_samples(self, n: int) -> torch.Tensor:
        """Gaussian directions from the Halton buffer, normalised (the reference's ``unit_ball`` samples)"""
        u = self.sampler.get_samples(n, bounded=False).clamp(1e-6, 1.0 - 1e-6)
        g = math.sqrt(2.0) * torch.erfinv(2.0 * u - 1.0)
        g = g / torch.norm(g, dim=-1, keepdim=True)
        if self.action_dim < 3:
            r = self.sampler.get_samples(n, bounded=False)[:, 0:1].clamp(0.0, 1.0)
            g = r * g
        return g

    def _feasible_subset(self, x: torch.Tensor, n: int) -> torch.Tensor:
        return x[self.feasibility.feasible(x)][:n]

    def generate_feasible_samples(self, n: int) -> torch.Tensor:
        x = self.sampler.get_samples(n + int(n * self.config.sample_rejection_ratio), bounded=True)
        return self._feasible_subset(x, n)

    def generate_feasible_samples_in_ellipsoid(self, x_start, x_goal, n: int, max_sampling_radius) -> torch.Tensor:
        ball = self._unit_ball_samples(n + int(n * self.config.sample_rejection_ratio))
        x = transform_unit_ball_to_ellipsoid_householder(x_start, x_goal, self.cspace_distance_weight, max_sampling_radius,
                                                         ball, self.low, self.high)
        return self._feasible_subset(x, n)

    def _extend(self, samples: torch.Tensor, neighbors_per_node: int) -> None:
        if samples.shape[0] == 0:
            return
        self._append(samples)
        self.connect_nodes(samples, neighbors_per_node)

    def extend_roadmap_with_random_samples(self, num_samples: int, neighbors_per_node: int = 10) -> None:
        self._extend(self.generate_feasible_samples(num_samples), neighbors_per_node)

    def extend_roadmap_with_ellipsoidal_samples(self, x_start, x_goal, max_sampling_radius, num_samples: int,
                                                neighbors_per_node: int = 5) -> None:
        self._extend(self.generate_feasible_samples_in_ellipsoid(x_start, x_goal, num_samples, max_sampling_radius),
                     neighbors_per_node)

    # ---- search (search/path_pruner.py)
    def _paths(self, si: List[int], gi: List[int]):
        res = [self.graph.shortest_path(s, g) for s, g in zip(si, gi)]
        return [r[0] for r in res], [r[1] for r in res]

    def _exists(self, si: List[int], gi: List[int]):
        lab = [self.graph.path_exists(s, g) for s, g in zip(si, gi)]
        return all(lab), lab

    @staticmethod
    def shortcut_edge_pairs(paths: List[List[int]]) -> List[Tuple[int, int]]:
        """every (path[i], path[j]) with j >= i of every path: the edges shortcut pruning steers (path_pruner.py:94-147)"""
        return [(p[i], p[j]) for p in paths for i in range(len(p)) for j in range(i, len(p))]

    def prune_path_with_shortcuts(self, paths, si, gi):
        pairs = self.shortcut_edge_pairs(paths)
        idx = torch.as_tensor(pairs, dtype=torch.int64, device=self.device)
        self.steer_and_register_edges(self._nodes[idx[:, 0]], self._nodes[idx[:, 1]], add_exact_node=False)
        return self._paths(si, gi)

    def check_samples_feasibility(self, q: torch.Tensor) -> torch.Tensor:
        return self.feasibility.feasible(q)

    # ---- queries (graph_planner_prm.py:259-515)
    def find_path(self, x_start: torch.Tensor, x_goal: torch.Tensor, interpolate_waypoints: bool = True,
                  interpolation_steps: int = 100, interpolation_type=None,
                  validate_interpolated_trajectory: bool = True) -> GraphPlannerResult:
        """x_start, x_goal [B, D] -> paths through the roadmap (``plan_waypoints``), with ``interpolated_waypoints``
        [B, interpolation_steps, D] (linear) when asked"""
        t0 = time.perf_counter()
        r = self._find_path_impl(x_start.to(self.device, torch.float32), x_goal.to(self.device, torch.float32))
        r.joint_names = self.joint_names
        if interpolate_waypoints and bool(r.success.any()):
            r.interpolated_waypoints = self.get_interpolated_trajectory(r.plan_waypoints, r.success, interpolation_steps)
            if validate_interpolated_trajectory:
                B = x_start.shape[0]
                ok = self.check_samples_feasibility(r.interpolated_waypoints.reshape(-1, self.action_dim))
                ok = ok.view(B, interpolation_steps).all(dim=1)
                r.success = ok & r.success
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        r.solve_time = time.perf_counter() - t0
        return r

    def _find_path_impl(self, x_start: torch.Tensor, x_goal: torch.Tensor) -> GraphPlannerResult:
        D, cfg = self.action_dim, self.config
        if x_start.ndim != 2 or x_goal.ndim != 2 or x_start.shape != x_goal.shape or x_start.shape[1] != D:
            raise ValueError(f"x_start and x_goal must both be [batch, {D}]")
        B = x_start.shape[0]
        res = GraphPlannerResult(success=torch.zeros(B, dtype=torch.bool, device=self.device),
                                 path_length=torch.full((B,), math.inf, device=self.device), plan_waypoints=[None] * B)
        if self._n > cfg.max_nodes * 0.75:
            self.reset_buffer()
        if not bool(self.check_samples_feasibility(torch.cat([x_start, x_goal], 0)).all()):
            res.valid_query = False
            res.debug_info = "Start or End state in collision"
            return res
        lin = self.weighted_distance(x_start, x_goal)
        if bool((lin < cfg.cspace_similarity_threshold).all()):
            res.success[:] = True
            res.plan_waypoints = [torch.stack([x_start[i], x_goal[i]]) for i in range(B)]
            res.path_length = lin
            return res
        s_nodes, g_nodes = self.initialize_terminal_graph_connections(x_start, x_goal)
        si = s_nodes[:, D].to(torch.int64).tolist()
        gi = g_nodes[:, D].to(torch.int64).tolist()
        exists, label = self._exists(si, gi)
        k_nn = cfg.neighbors_per_node
        if exists:
            g_path, lengths = self._paths(si, gi)
            if max(len(p) for p in g_path) > 2:
                g_path, lengths = self.prune_path_with_shortcuts(g_path, si, gi)
                label = [len(p) <= 3 for p in g_path]
            if max(len(p) for p in g_path) <= 2:
                g_path = [p if len(p) > 1 else [p[0], p[0]] for p in g_path]
                res.plan_waypoints = self.get_nodes_in_path(g_path)
                res.success = torch.as_tensor(label, dtype=torch.bool, device=self.device)
                res.path_length = torch.as_tensor(lengths, dtype=torch.float32, device=self.device)
                return res
        c_max = lin.view(-1) * cfg.exploration_radius
        n_new = cfg.new_nodes_per_iteration
        finetune, it = 0, 0
        while not exists or finetune < cfg.min_finetune_iterations:
            todo = label if all(label) else [not x for x in label]
            i = self._rng.choice([j for j, x in enumerate(todo) if x])
            self.extend_roadmap_with_ellipsoidal_samples(x_start[i], x_goal[i], c_max[i], n_new, k_nn)
            it += 1
            exists, label = self._exists(si, gi)
            if exists:
                g_path, lengths = self._paths(si, gi)
                if max(len(p) for p in g_path) > 2:
                    g_path, lengths = self.prune_path_with_shortcuts(g_path, si, gi)
                label = [len(p) <= 3 for p in g_path]
                finetune += 1
                if max(len(p) for p in g_path) <= 2:
                    break
                c_max[:] = torch.as_tensor(lengths, dtype=torch.float32, device=self.device)
            else:
                c_max[i] = c_max[i] * cfg.exploration_radius_growth_factor
            k_nn = int(cfg.neighbors_per_node_growth_factor * k_nn)
            n_new = int(cfg.new_nodes_per_iteration_growth_factor * n_new)
            if it >= cfg.max_path_finding_iterations:
                break
        exists, label = self._exists(si, gi)
        if not exists:
            g_path, lengths = [None] * B, [math.inf] * B
            ok = [j for j, x in enumerate(label) if x]
            if ok:
                p, _ = self._paths([si[j] for j in ok], [gi[j] for j in ok])
                p, c = self.prune_path_with_shortcuts(p, [si[j] for j in ok], [gi[j] for j in ok])
                for n, j in enumerate(ok):
                    g_path[j], lengths[j] = p[n], c[n]
        else:
            g_path, lengths = self._paths(si, gi)
            if max(len(p) for p in g_path) > 3:
                g_path, lengths = self.prune_path_with_shortcuts(g_path, si, gi)
        g_path = [None if p is None else (p if len(p) > 1 else [p[0], p[0]]) for p in g_path]
        res.plan_waypoints = self.get_nodes_in_path(g_path)
        res.success = torch.as_tensor(label, dtype=torch.bool, device=self.device)
        res.path_length = torch.as_tensor(lengths, dtype=torch.float32, device=self.device)
        return res

    def get_interpolated_trajectory(self, paths, success: torch.Tensor, interpolation_steps: int) -> torch.Tensor:
        """linear interpolation of each successful path's waypoints to ``interpolation_steps`` points
        (graph_planner_prm.py:516-563, util/trajectory.py linear_smooth): waypoint i sits at step i (n - 1) / (P - 1)"""
        out = np.zeros((len(paths), interpolation_steps, self.action_dim), np.float32)
        for b in torch.nonzero(success).view(-1).tolist():
            out[b] = linear_interpolate_waypoints(paths[b].detach().cpu().numpy().reshape(-1, self.action_dim), interpolation_steps)
        return torch.as_tensor(out, device=self.device)

    def warmup(self, x_start: Optional[torch.Tensor] = None, x_goal: Optional[torch.Tensor] = None) -> None:
        if x_start is not None and x_goal is not None:
            self.find_path(x_start, x_goal)
        self.reset_buffer()


def linear_interpolate_waypoints(waypoints: np.ndarray, n: int) -> np.ndarray:
    """waypoints [P >= 2, D] -> [n, D]: piecewise linear, waypoint i at step i (n - 1) / (P - 1)"""
    P = waypoints.shape[0]
    if P < 2:
        raise ValueError("a path has at least two waypoints")
    y = np.arange(P, dtype=np.float64) * (float(n - 1) / float(P - 1))
    t = np.arange(n, dtype=np.float64)
    return np.stack([np.interp(t, y, waypoints[:, d]) for d in range(waypoints.shape[1])], axis=1).astype(np.float32)
