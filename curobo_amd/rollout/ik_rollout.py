"""Teleport (horizon 1) rollout for inverse kinematics: q -> FK -> tool-pose + c-space bound +
self + scene collision costs, and the analytic gradient back to q.

Data path of the reference's ``RobotRollout`` with ``StateFromPositionTeleport``
(``content/configs/task/ik/transition_ik.yml``) and the IK cost set
(``content/configs/task/ik/lbfgs_ik.yml:3-36``); kernels cited in the backend modules.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from ..backends import cost as cost_hip
from ..backends import rollout as rollout_hip
from ..cost import support_polygon
from ..robot.kinematics_params import KinematicsParams
from ..scene.data import SceneData
from .base import PoseTerms, RobotRolloutBase


@dataclass
class IKRolloutCfg:
    """Defaults = reference ``lbfgs_ik.yml``."""

    pose_weight: List[float] = field(default_factory=lambda: [10000.0, 500.0])
    pose_convergence_tolerance: List[float] = field(default_factory=lambda: [1e-8, 1e-8])
    rotation_method: int = 0  # use_lie_group: false
    cspace_weight: List[float] = field(default_factory=lambda: [5000.0, 0.0])
    cspace_activation_distance: List[float] = field(default_factory=lambda: [0.01, 0.01])
    scene_collision_weight: float = 5000.0
    scene_activation_distance: float = 0.0
    self_collision_weight: float = 5000.0
    #: one fused launch (csrc/rollout_ik_fused.hip, rollout_ik_fused_kernel) for cost + gradient when 16
    #: configurations fit in LDS; False = the seven drop-in launches
    use_fused: bool = True
    #: weight of the support-polygon (balance) term: the centre of mass' xy against the polygon of ``update_support_polygon``
    #: (reference CostSupportPolygon); 0 = off, the launches are then exactly those without it.  Positive: the kernel sequence
    #: runs (FK with the centre of mass, csrc/support_polygon.hip, the FK VJP with its gradient), not the fused launch.
    support_polygon_weight: float = 0.0
    #: the reference's ``inside_cost_weight``: a small pull towards the middle of the polygon while inside (0: no cost inside)
    support_polygon_inside_cost_weight: float = 0.001
    #: weights of the implied velocity / acceleration regularisation w.r.t. the current state (reference
    #: ``squared_l2_regularization_weight`` of the c-space position cost, cost_cspace_cfg.py); read by a rollout built with
    #: ``use_current_state=True``
    squared_l2_regularization_weight: List[float] = field(default_factory=lambda: [0.0, 0.0])


#: rows of a support polygon's fixed buffer (the cost launch's limit)
SUPPORT_POLYGON_CAPACITY = support_polygon.MAX_HULL_VERTICES


class IKRollout(PoseTerms, RobotRolloutBase):
    """cost[B] and d cost / d q [B, D] for B joint configurations against per-row goal poses."""

    def __init__(self, kin: KinematicsParams, scene: Optional[SceneData], batch_size: int,
                 cfg: Optional[IKRolloutCfg] = None, num_goalset: int = 1, use_current_state: bool = False):
        """``use_current_state``: the c-space term is taken w.r.t. a current state (``update_current_state``): joint limits
        tightened to one time step from it + ``cfg.squared_l2_regularization_weight``.  Such a rollout always launches the
        state variant of the fused launch / passes the state to the c-space kernel; ``dt`` = 0 (the initial state) gives the
        plain term from the same launches."""
        c = cfg or IKRolloutCfg()
        super().__init__(kin, scene, c, c.self_collision_weight, c.scene_collision_weight, c.scene_activation_distance)
        self.action_horizon = 1
        self.num_goalset = num_goalset
        d, D = self.device, kin.num_dof
        f = lambda v: torch.tensor(v, device=d, dtype=torch.float32)  # noqa: E731
        self._init_pose_terms(c.pose_weight, c.pose_convergence_tolerance, None)
        self._cs_w, self._cs_eta = f(c.cspace_weight), f(c.cspace_activation_distance)
        self._p_b = kin.joint_limits_position.contiguous()
        self._effort_b = torch.stack([torch.full((D,), -1e9, device=d), torch.full((D,), 1e9, device=d)])
        self._v_b = kin.joint_limits_velocity.contiguous()
        self._zero1 = torch.zeros(1, device=d)
        self._zeroD = torch.zeros(1, D, device=d)
        self._onesD = torch.ones(D, device=d)
        self._reg = torch.zeros(2, device=d)
        self.use_current_state = bool(use_current_state)
        if self.use_current_state:
            self._reg = f(c.squared_l2_regularization_weight)
            self._acc_reg = float(c.squared_l2_regularization_weight[1]) > 0.0
            self._cur_pos, self._cur_vel, self._state_dt = torch.zeros(1, D, device=d), torch.zeros(1, D, device=d), torch.zeros(1, device=d)
        self._env_runs_ok = True  # env_query_idx constant over aligned runs of 16 rows (update_env_query_idx)
        self._use_support_polygon = float(c.support_polygon_weight) > 0.0
        if self._use_support_polygon:
            self._w_sp = f([c.support_polygon_weight])
            self._sp_hulls, self._sp_counts, self._sp_set = None, None, False
        self.update_batch_size(batch_size)

    def _alloc(self, B: int) -> None:
        self._alloc_robot_buffers(B, 1)
        self._alloc_pose_buffers(B, 1, self.num_goalset)
        self.cspace_cost, self.cspace_grad = self._zeros(B, 1, self.action_dim), self._zeros(B, 1, self.action_dim)
        if self._use_support_polygon:
            self.sp_cost, self.sp_grad, self.sp_distance = self._zeros(B, 1), self._zeros(B, 1, 4), self._zeros(B, 1)
            self._sp_idxs = self._zeros(B, dt=torch.int32)
        self._idxs_src = None  # (the row -> goal map was reallocated: the next update_goals must copy, whatever tensor it is handed)
        self._idxs_cur, self._idxs_cur_src = self._zeros(B, dt=torch.int32), None  # row -> current state

    def update_env_query_idx(self, env_query_idx: Optional[torch.Tensor]) -> None:
        """Scene environment of every configuration (see the base).  The fused IK launch serves 16 configurations per
        workgroup from one staged scene / sphere set: it runs when the index is constant over aligned runs of 16 rows (the
        seeds of one problem; checked here, one host read-back, never inside a captured launch sequence), else the kernel
        sequence does.  Switching modes changes the launches: re-capture graphs."""
        super().update_env_query_idx(env_query_idx)
        self._env_runs_ok = True
        if env_query_idx is not None:
            idx = self.env_query_idx
            first = idx[(torch.arange(idx.numel(), device=idx.device) // 16) * 16]
            self._env_runs_ok = bool((idx == first).all())

    def update_goals(self, goal_position: torch.Tensor, goal_quat: torch.Tensor, idxs_goal: torch.Tensor) -> None:
        """goal_position [G, T, num_goalset, 3], goal_quat (wxyz) [G, T, num_goalset, 4], idxs_goal [B]."""
        assert goal_position.shape[1:3] == (self.kin.num_pose_links, self.num_goalset)
        self._update_goal_poses(goal_position, goal_quat)
        key = (idxs_goal, idxs_goal._version)  # (solvers pass the same, unmodified row -> goal map every solve: no copy then)
        last = self._idxs_src
        if last is None or last[0] is not key[0] or last[1] != key[1]:
            self.idxs_goal.copy_(idxs_goal.to(torch.int32))
            self._idxs_src = key

    def update_current_state(self, position: torch.Tensor, velocity: Optional[torch.Tensor] = None, dt=None,
                             idxs: Optional[torch.Tensor] = None) -> None:
        """position [P, D], velocity [P, D] or None (= at rest), dt [P] / float / None, idxs [B]: row b is taken w.r.t. state
        idxs[b] (kept when None).  Copied into fixed buffers, so captured graphs stay valid as long as P does not change (a new
        P allocates: re-capture).  ``dt`` None or 0 writes zeros: the terms are off, the launches are the same."""
        if not self.use_current_state:
            raise ValueError("update_current_state: the rollout was built without use_current_state=True")
        d, D = self.device, self.action_dim
        p = position.to(d, torch.float32).reshape(-1, D)
        if p.shape != self._cur_pos.shape:
            self._cur_pos, self._cur_vel, self._state_dt = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(p.shape[0], device=d)
            self._idxs_cur.zero_()  # (indices into the old states may be out of range now)
            self._idxs_cur_src = None
        P = self._cur_pos.shape[0]
        if idxs is not None:
            key = (idxs, idxs._version)  # (solvers pass the same, unmodified row -> problem map every solve: no copy, no check then)
            last = self._idxs_cur_src
            if last is None or last[0] is not key[0] or last[1] != key[1]:
                if idxs.numel() != self.batch_size or int(idxs.min()) < 0 or int(idxs.max()) >= P:
                    raise ValueError(f"update_current_state: idxs must hold {self.batch_size} state indices in [0, {P})")
                self._idxs_cur.copy_(idxs.to(device=d, dtype=torch.int32).reshape(-1))
                self._idxs_cur_src = key
        self._cur_pos.copy_(p)
        self._cur_vel.copy_(velocity.to(d, torch.float32).reshape(P, D)) if velocity is not None else self._cur_vel.zero_()
        if dt is None:
            self._state_dt.zero_()
        elif torch.is_tensor(dt):
            self._state_dt.copy_(dt.to(d, torch.float32).reshape(-1).expand(P))
        else:
            self._state_dt.fill_(float(dt))

    def update_support_polygon(self, vertices_xy: torch.Tensor, idxs: Optional[torch.Tensor] = None,
                               padding: float = support_polygon.DEFAULT_PADDING) -> None:
        """vertices_xy [P, n, 2] (3 <= n <= 64: e.g. the xy of the foot spheres of P stances), idxs [B]: row b is held over
        polygon idxs[b] (kept when None; all rows over polygon 0 at first).  One launch builds the P hulls (padded by ``padding``)
        into a buffer of SUPPORT_POLYGON_CAPACITY rows per polygon plus their vertex counts, so a captured graph stays valid
        when the polygon changes, as long as P does not (a new P allocates: re-capture).  Never call it inside a capture."""
        if not self._use_support_polygon:
            raise ValueError("update_support_polygon: the rollout was built with support_polygon_weight = 0")
        v = torch.as_tensor(vertices_xy).to(self.device, torch.float32)
        if v.dim() != 3 or v.shape[-1] != 2:
            raise ValueError(f"update_support_polygon: vertices_xy must be (P, n, 2), got {tuple(v.shape)}")
        P, n, cap = int(v.shape[0]), int(v.shape[1]), SUPPORT_POLYGON_CAPACITY
        hulls, counts = support_polygon.convex_hulls(v, padding)
        if n > cap and int(counts.max()) > cap:
            raise ValueError(f"update_support_polygon: a hull has {int(counts.max())} vertices, at most {cap} fit")
        if self._sp_hulls is None or self._sp_hulls.shape[0] != P:
            self._sp_hulls, self._sp_counts = self._zeros(P, cap, 2), self._zeros(P, dt=torch.int32)
            self._sp_idxs.zero_()  # (indices into the old polygons may be out of range now)
        self._sp_hulls[:, :min(n, cap)].copy_(hulls[:, :cap])
        self._sp_counts.copy_(counts)
        if idxs is not None:
            if idxs.numel() != self.batch_size or int(idxs.min()) < 0 or int(idxs.max()) >= P:
                raise ValueError(f"update_support_polygon: idxs must hold {self.batch_size} polygon indices in [0, {P})")
            self._sp_idxs.copy_(idxs.to(device=self.device, dtype=torch.int32).reshape(-1))
        self._sp_set = True

    def _support_polygon_term(self) -> None:
        """com -> sp_cost [B, 1], sp_grad [B, 1, 4] (weighted, what the FK VJP takes) and sp_distance [B, 1]"""
        if not self._sp_set:
            raise ValueError("support_polygon_weight > 0 but no polygon is set: call update_support_polygon first")
        cost_hip.support_polygon_cost(self.sp_cost, self.sp_grad, self.sp_distance, self.com, self._sp_hulls, self._sp_counts,
                                      self._sp_idxs, self._w_sp, self.cfg.support_polygon_inside_cost_weight,
                                      support_polygon.MARGIN_TARGET, support_polygon.SMOOTHING)

    def _state_args(self):
        """(regularisation weights, current position, current velocity, row -> state, dt per state) of the c-space term; without
        a current state: the zeros that switch the terms off"""
        if self.use_current_state:
            return self._reg, self._cur_pos, self._cur_vel, self._idxs_cur, self._state_dt
        return self._reg, self._zeroD, self._zeroD, self._idx0, self._zero1

    # ------------------------------------------------------------------ forward + backward
    def evaluate(self, q: torch.Tensor, with_gradient: bool = True) -> torch.Tensor:
        k, B = self.kin, self.batch_size
        T, S, D = k.num_pose_links, k.num_spheres, k.num_dof
        sp = self._use_support_polygon
        self._fk_forward(q, compute_com=sp)
        self._pose_term()
        reg, cur_pos, cur_vel, idxs_cur, state_dt = self._state_args()
        cost_hip.cspace_position_cost(
            self.cspace_cost, self.cspace_grad, None, q, None, self._zeroD, self._idx0, self._p_b, self._effort_b,
            self._cs_w, self._cs_eta, self._zero1, self._onesD, reg, cur_pos, cur_vel, idxs_cur,
            self._v_b, state_dt, True, B, 1, D)
        self._self_collision()
        use_scene = self.scene is not None
        if use_scene:
            self._scene_collision()
        if sp:
            self._support_polygon_term()
            if with_gradient:
                self._fk_backward(self.pose_grad_pos, self.pose_grad_quat, self.self_grad, self.scene_grad if use_scene else None,
                                  grad_com=self.sp_grad)
            cost_hip.rollout_point_aggregate_terms(
                self.cost, self.grad_q if with_gradient else None, self.pose_cost, self.cspace_cost,
                self.cspace_grad if with_gradient else None, self.self_dist, self.scene_dist if use_scene else None,
                self.sp_cost, B, T, D, S)
            return self.cost
        if with_gradient:
            self._fk_backward(self.pose_grad_pos, self.pose_grad_quat, self.self_grad, self.scene_grad if use_scene else None)
        cost_hip.rollout_point_aggregate(
            self.cost, self.grad_q if with_gradient else None, self.pose_cost, self.cspace_cost,
            self.cspace_grad if with_gradient else None, self.self_dist, self.scene_dist if use_scene else None, B, T,
            D, S)
        return self.cost

    # ------------------------------------------------------------------ fused
    def fused_available(self) -> bool:
        k = self.kin
        return k.num_dof <= 64 and self._fused_fits(rollout_hip.rollout_ik_fused_lds_bytes(
            k.num_dof, k.num_links, k.num_spheres, int(k.self_collision.collision_pairs.shape[0]),
            int(k.link_chain_data.shape[0]), self._obstacle_slots()))

    def cost_and_gradient_fused(self, q: torch.Tensor, with_metrics: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Same numbers as ``evaluate`` from one launch; ``with_metrics`` also fills the pose-error,
        link-pose and sphere buffers the solver's metrics read."""
        k, B, c = self.kin, self.batch_size, self.cfg
        sc = k.self_collision
        m = with_metrics
        state = {}
        if self.use_current_state:  # curobo_hip_rollout_ik_fused_state
            state = dict(squared_l2_reg_weight=self._reg, current_position=self._cur_pos, current_velocity=self._cur_vel,
                         idxs_current_state=self._idxs_cur, velocity_limits=self._v_b, state_dt=self._state_dt,
                         acceleration_regularization=self._acc_reg)
        rollout_hip.rollout_ik_fused(
            self.cost, self.grad_q, self.pose_cost if m else None, self.pose_pos_dist if m else None,
            self.pose_rot_dist if m else None, self.goalset_idx if m else None, self.link_pos if m else None,
            self.link_quat if m else None, self.robot_spheres if m else None, self.cspace_cost if m else None,
            q, self.goal_position, self.goal_quat, self.idxs_goal, self._pose_w, self._axes_w, self._tol, self._project,
            self.num_goalset, c.rotation_method, self._p_b, self._cs_w, self._cs_eta, k.fixed_transforms, k.link_spheres,
            k.joint_map_type, k.joint_map, k.link_map, k.tool_frame_map, k.link_sphere_idx_map, k.link_chain_data,
            k.link_chain_offsets, k.joint_offset_map, sc.sphere_padding, self._w_self, sc.collision_pairs,
            self.scene.struct if self.scene is not None else None, self._w_scene, self._eta_scene, B, k.num_dof,
            self.env_query_idx, k.num_envs, self.use_multi_env, **state)
        return self.cost, self.grad_q.view(B, -1)

    def cost_and_gradient(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x[B, D] -> (cost[B], grad[B, D]) in static buffers (graph friendly)."""
        if (self.cfg.use_fused and not self._use_support_polygon and (self._env_runs_ok or not (self.use_multi_env or self.kin.num_envs > 1))
                and self._fused_chosen()):
            return self.cost_and_gradient_fused(x.view(self.batch_size, self.action_dim).contiguous())
        cost = self.evaluate(x.view(self.batch_size, 1, self.action_dim), with_gradient=True)
        return cost, self.grad_q.view(self.batch_size, -1)
