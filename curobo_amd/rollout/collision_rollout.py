"""The rollout hot path: knots -> B-spline -> FK -> self + scene collision -> per-trajectory cost,
and the analytic backward to the knots, as one straight line of kernel launches.

This is the data path of the reference's ``RobotRollout.evaluate_action`` followed by
``cost.backward`` (``curobo/_src/rollout/rollout_robot.py:252-263,537-587`` and
``optim/components/gradient_opt_core.py:445-480``; call stack in SURVEY.md section 3.2) with the
collision cost terms of ``content/configs/task/trajopt/lbfgs_bspline_trajopt.yml:44-53``.  The
reference builds a torch autograd graph (one ``autograd.Function`` per kernel, extra torch kernels
for ``zero_()``, gradient scaling, sphere-gradient add and ``cat_sum``); here forward and VJP are
explicit launches on pre-allocated buffers -- nothing is allocated, synchronised or read back, so
the whole evaluation is hipGraph-capturable, and the two sphere-gradient buffers are summed inside
the FK backward kernel instead of by an elementwise add.

``curobo_amd.hip_ops`` holds the drop-in ``autograd.Function`` wrappers for callers that need
the reference's autograd contract; tests check both paths give the same numbers.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..backends import collision as collision_hip
from ..backends import rollout as rollout_hip
from ..robot.kinematics_params import KinematicsParams
from ..scene.data import SceneData
from .base import BSplineHorizon, BSplineRolloutBase


@dataclass
class CollisionRolloutCfg(BSplineHorizon):
    """Defaults follow the reference trajopt task (weights/activation: lbfgs_bspline_trajopt.yml
    :44-53; control space BSPLINE_3 with the BASELINE C2 shape: 12 knots x 2 interpolation steps
    -> horizon 32, padded 33)."""

    n_knots: int = 12
    interpolation_steps: int = 2
    bspline_degree: int = 3
    traj_dt: float = 0.05
    self_collision_weight: float = 10000.0
    scene_collision_weight: float = 100000.0
    activation_distance: float = 0.0025
    use_sweep: bool = True
    use_speed_metric: bool = True
    use_self_collision: bool = True
    use_scene_collision: bool = True
    #: one fused launch (csrc/rollout_fused.hip) instead of the 7-kernel sequence whenever one
    #: trajectory fits in LDS; False forces the drop-in kernel sequence (and materialises every
    #: intermediate tensor, which the fused path only does on request)
    use_fused: bool = True
    # fused launches map workgroups to trajectories longest-first (durations measured by the previous
    # launch; same outputs, shorter launch tail when trajectories differ in collision work)
    longest_first_dispatch: bool = True
    #: fused path: also write position[B,H,D] and robot_spheres[B,H,S,4] to HBM
    fused_materialize: bool = False
    #: compile a compile-time shape of the fused launch for THIS robot / horizon at first use when the library holds none
    #: (``backends/fused_jit.py``: hipcc at run time, 5-10 s once, cached on disk -- the reference compiles its kernels per robot
    #: with NVRTC); also switched on by CUROBO_HIP_JIT_SHAPES=1.  Same results, ~20 % faster launches.
    jit_shape: bool = False


class CollisionRollout(BSplineRolloutBase):
    """Cost and gradient of ``batch_size`` B-spline trajectories (one "rollout" each)."""

    def __init__(self, kin: KinematicsParams, scene: Optional[SceneData], batch_size: int,
                 cfg: Optional[CollisionRolloutCfg] = None):
        cfg = cfg or CollisionRolloutCfg()
        super().__init__(kin, scene, cfg, cfg.self_collision_weight, cfg.scene_collision_weight, cfg.activation_distance)
        self._eta = self._eta_scene
        self.update_batch_size(batch_size)
        self.update_start_state(None)

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int) -> None:
        H, T, z = self.cfg.padded_horizon, self.kin.num_pose_links, self._zeros
        self._alloc_bspline_buffers(B)
        self._alloc_robot_buffers(B, H)
        self._pair_distance = self._pd
        self.grad_zero_pos, self.grad_zero_quat = z(B, H, T, 3), z(B, H, T, 4)
        self.grad_zero_state = z(B, H, self.action_dim)

    @property
    def _use_self(self) -> bool:
        return self.cfg.use_self_collision

    @property
    def _use_scene(self) -> bool:
        return self.cfg.use_scene_collision and self.scene is not None

    def update_start_state(self, start_position: Optional[torch.Tensor]) -> None:
        """One shared start state (position; zero velocity/acceleration/jerk)."""
        super().update_start_state(start_position)

    # ------------------------------------------------------------------ forward
    def compute_state_from_action(self, act_seq: torch.Tensor) -> torch.Tensor:
        self._bspline_forward(act_seq)
        return self.position

    def compute_kinematics(self, q: torch.Tensor) -> torch.Tensor:
        self._fk_forward(q)
        return self.robot_spheres

    def compute_costs(self) -> torch.Tensor:
        cfg, sc = self.cfg, self.kin.self_collision
        if self._use_self:
            self._self_collision(sc.num_blocks_per_batch, sc.max_threads_per_block)
        if self._use_scene:
            self._scene_collision(cfg.use_sweep, cfg.use_speed_metric, self._speed_dt)
        collision_hip.trajectory_cost_sum(
            self.cost, self.self_dist if self._use_self else None, self.scene_dist if self._use_scene else None,
            self.batch_size, cfg.padded_horizon, self.kin.num_spheres)
        return self.cost

    def evaluate_action(self, act_seq: torch.Tensor) -> torch.Tensor:
        """cost[B] of ``act_seq[B, n_knots, D]`` (reference RobotRollout.evaluate_action)."""
        self.compute_kinematics(self.compute_state_from_action(act_seq))
        return self.compute_costs()

    # ------------------------------------------------------------------ reference Rollout protocol
    # (curobo/_src/rollout/rollout_protocol.py:46-174): the members solvers and optimisers rely on
    @property
    def action_bound_lows(self) -> torch.Tensor:
        return self.kin.joint_limits_position[0]

    @property
    def action_bound_highs(self) -> torch.Tensor:
        return self.kin.joint_limits_position[1]

    @property
    def dt(self) -> float:
        return self.cfg.traj_dt

    @property
    def sum_horizon(self) -> bool:
        return True  # costs are returned summed over the horizon, one value per trajectory

    def compute_metrics_from_action(self, act_seq: torch.Tensor) -> dict:
        """reference :107-121: evaluate through the kernel sequence (materialised state) and report
        per-trajectory metrics: cost, worst self / scene collision terms, feasibility."""
        with torch.no_grad():
            cost = self.evaluate_action(act_seq.view(self.batch_size, self.cfg.n_knots, self.action_dim)).clone()
        B = self.batch_size
        self_c = self.self_dist.view(B, -1).sum(-1) if self.cfg.use_self_collision else torch.zeros_like(cost)
        scene_on = self.cfg.use_scene_collision and self.scene is not None
        scene_c = self.scene_dist.view(B, -1).sum(-1) if scene_on else torch.zeros_like(cost)
        return {"cost": cost, "self_collision_cost": self_c.clone(), "scene_collision_cost": scene_c.clone(),
                "feasible": (self_c + scene_c) == 0.0, "position": self.position}

    def update_params(self, start_position: Optional[torch.Tensor] = None, scene: Optional[SceneData] = None,
                      env_query_idx: Optional[torch.Tensor] = None) -> bool:
        """reference :123-129 (goal / start / world updates between solves, buffers stay in place)"""
        if start_position is not None:
            self.update_start_state(start_position)
        if scene is not None:
            self.scene = scene
            self._fused_ok = None
        if env_query_idx is not None:
            self.update_env_query_idx(env_query_idx)
        return True

    def reset(self, **kwargs) -> bool:
        return True

    def reset_shape(self) -> bool:
        return True

    def reset_seed(self) -> None:
        return None

    # ------------------------------------------------------------------ backward
    def backward(self) -> torch.Tensor:
        """d(sum cost)/d(knots) of the last ``evaluate_action`` (grad_output = 1 per trajectory,
        the reference's ``cost.backward(gradient=self._l_vec)`` with ``_l_vec`` = ones)."""
        ga = self.self_grad if self._use_self else (self.scene_grad if self._use_scene else None)
        gb = self.scene_grad if (self._use_self and self._use_scene) else None
        self._fk_backward(self.grad_zero_pos, self.grad_zero_quat, ga, gb)
        self._bspline_backward(self.grad_zero_state, self.grad_zero_state, self.grad_zero_state)
        return self.grad_knots

    # ------------------------------------------------------------------ fused
    def fused_available(self) -> bool:
        cfg, k = self.cfg, self.kin
        n_pairs = k.self_collision.collision_pairs.shape[0] if self._use_self else 0
        return self._fused_fits(rollout_hip.rollout_trajectory_fused_lds_bytes(
            cfg.padded_horizon, self.action_dim, k.num_links, k.num_spheres, n_pairs, int(k.link_chain_data.shape[0]),
            self._obstacle_slots()))

    def _reuse_launch_ok(self) -> bool:
        return self.cfg.use_fused and not self.cfg.fused_materialize and self._fused_chosen()

    def cost_and_gradient_fused(self, act_seq: torch.Tensor, memo: Optional[tuple] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Same numbers as ``evaluate_action`` + ``backward`` from one kernel launch.  ``memo = (x, cost, grad, stride[, slot])``:
        evaluations the caller holds (``offers_reuse``; ``backends.rollout.rollout_trajectory_fused``)."""
        cfg, k, B = self.cfg, self.kin, self.batch_size
        use_self, use_scene = self._use_self, self._use_scene
        sc = k.self_collision
        mat = cfg.fused_materialize
        rollout_hip.rollout_trajectory_fused(
            self.cost, self.grad_knots, self.position if mat else None, self.robot_spheres if mat else None,
            act_seq, *self._bspline_args(), k.fixed_transforms, k.link_spheres, k.joint_map_type, k.joint_map, k.link_map,
            k.link_sphere_idx_map, k.link_chain_data, k.link_chain_offsets, k.joint_offset_map,
            sc.sphere_padding, self._w_self if use_self else None, sc.collision_pairs if use_self else None,
            self.scene.struct if use_scene else None, self._w_scene if use_scene else None,
            self._eta, self._speed_dt, self.env_query_idx, k.num_envs, self.use_multi_env, B, cfg.padded_horizon,
            self.action_dim, cfg.n_knots, cfg.bspline_degree, 3 if cfg.use_sweep else 0,
            cfg.use_sweep and cfg.use_speed_metric, self._dispatch_order(), memo=self._checked_memo(memo))
        return self.cost, self.grad_knots

    def cost_and_gradient(self, x: torch.Tensor, memo: Optional[tuple] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """x[B, n_knots*D] -> (cost[B], grad[B, n_knots*D]); buffers are reused every call.  Without ``memo`` every
        trajectory is evaluated; with it (only where ``offers_reuse``) the rows the caller holds are copied."""
        act = x.view(self.batch_size, self.cfg.n_knots, self.action_dim)
        if self.cfg.use_fused and self._fused_chosen():
            cost, grad = self.cost_and_gradient_fused(act, memo=memo)
            return cost, grad.view(self.batch_size, -1)
        self._checked_memo(memo)
        cost = self.evaluate_action(act)
        grad = self.backward()
        return cost, grad.view(self.batch_size, -1)

    # ------------------------------------------------------------------ accounting
    def algorithmic_bytes_per_point(self) -> int:
        """8D + 56T + 96L + 84S + 4 (API-materialised tensors, fp32)."""
        k = self.kin
        return 8 * k.num_dof + 56 * k.num_pose_links + 96 * k.num_links + 84 * k.num_spheres + 4
