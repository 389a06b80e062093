"""What the robot rollouts share: the robot buffers, the environment index, one method per kernel launch and the choice between
the fused launch and the kernel sequence (``RobotRolloutBase``); the B-spline state, its two launches and the fused launch's
dispatch / compile-time-shape helpers of the two trajectory rollouts (``BSplineRolloutBase``); the tool-pose term of the IK and
trajopt rollouts (``PoseTerms``).

Every launch of ``backends`` that a rollout makes is spelled out here once, with the robot model's tensors taken from ``self.kin``;
the rollouts pass what varies between them.  ``solver/trajopt.py``'s interpolated check is a ``RobotRolloutBase`` without a gradient.
"""

from __future__ import annotations

from typing import Optional

import torch

from ..backends import collision as collision_hip
from ..backends import cost as cost_hip
from ..backends import geometry as geometry_hip
from ..backends import kinematics as kinematics_hip
from ..backends import rollout as rollout_hip
from ..backends import trajectory as trajectory_hip
from ..robot.kinematics_params import KinematicsParams
from ..scene.data import SceneData, validate_env_query_idx


def obstacle_slots(scene: Optional[SceneData]) -> int:
    """obstacle records per environment that a fused launch stages in LDS (cuboids + voxel grids; 0 without a scene)"""
    return 0 if scene is None else scene.struct.max_cuboids + scene.struct.max_voxel_grids


def scene_has_meshes(scene: Optional[SceneData]) -> bool:
    """mesh obstacles are queried by their own launch (BVH): a scene that holds some runs the kernel sequence"""
    return scene is not None and getattr(scene.struct, "mesh_set", None) is not None


def fk_forward_spheres(kin: KinematicsParams, link_pos, link_quat, robot_spheres, com, cumul_mat, q, env_query_idx,
                       n_points: int, horizon: int, compute_com: bool = False) -> None:
    """q [n_points, D] -> tool-frame poses, spheres and the cumulative link transforms; ``compute_com``: also the centre of
    mass (xyz + total mass) into ``com``, which the launch leaves untouched otherwise"""
    k = kin
    kinematics_hip.launch_kinematics_forward_spheres(
        link_pos, link_quat, robot_spheres, com, cumul_mat, q, k.fixed_transforms, k.link_spheres, k.link_masses_com,
        k.joint_map_type, k.joint_map, k.link_map, k.tool_frame_map, k.link_sphere_idx_map, k.joint_offset_map, env_query_idx,
        k.num_envs, n_points, horizon, k.num_dof, k.num_spheres, 32, True, compute_com)


class BSplineHorizon:
    """``horizon`` / ``padded_horizon`` of a Cfg dataclass with ``n_knots``, ``bspline_degree`` and ``interpolation_steps``"""

    @property
    def horizon(self) -> int:
        return (self.n_knots + self.bspline_degree + 1) * self.interpolation_steps

    @property
    def padded_horizon(self) -> int:
        return self.horizon + 1


class RobotRolloutBase:
    """``batch_size`` rows of ``_H`` points each: FK -> self + scene collision, and the FK backward."""

    def __init__(self, kin: KinematicsParams, scene: Optional[SceneData], cfg, self_collision_weight: float,
                 scene_collision_weight: float, scene_activation_distance: float):
        self.kin, self.scene, self.cfg = kin, scene, cfg
        self.device, self.action_dim = kin.device, kin.num_dof
        self.batch_size, self._H = 0, 0
        self.use_multi_env = False
        self._fused_ok: Optional[bool] = None
        self._dispatch = None
        f = lambda v: torch.tensor([v], device=self.device, dtype=torch.float32)  # noqa: E731
        self._w_self, self._w_scene = f(self_collision_weight), f(scene_collision_weight)
        self._eta_scene = f(scene_activation_distance)

    # ------------------------------------------------------------------ buffers
    def _zeros(self, *shape, dt=torch.float32) -> torch.Tensor:
        return torch.zeros(*shape, device=self.device, dtype=dt)

    def update_batch_size(self, batch_size: int) -> None:
        if batch_size == self.batch_size:
            return
        # (the dispatch workspace is sized for the batch, and the choice between the fused launch and the kernel sequence may
        # depend on it)
        self._dispatch = self._fused_ok = None
        self._alloc(batch_size)

    def _alloc_robot_buffers(self, B: int, H: int) -> None:
        k, z = self.kin, self._zeros
        S, L, T = k.num_spheres, k.num_links, k.num_pose_links
        self.batch_size, self._H = B, H
        # kinematics (reference KinematicsFusedFunction.create_buffers, cuda_ops/kinematics.py:27-90)
        self.link_pos, self.link_quat = z(B, H, T, 3), z(B, H, T, 4)
        self.robot_spheres, self.cumul_mat, self.com = z(B, H, S, 4), z(B, H, L, 3, 4), z(B, H, 4)
        self.env_query_idx = z(B, dt=torch.int32)
        # self collision (reference SelfCollisionCost.setup_batch_tensors, cost/cost_self_collision.py:31-89)
        self.self_dist, self.self_grad, self.self_sparse = z(B, H, 1), z(B, H, S, 4), z(B, H, S, dt=torch.uint8)
        self._pd, self._bbmv, self._bbmi = z(1), z(1), z(2, dt=torch.int16)
        # scene collision (reference CollisionBuffer, geom/collision/buffer_collision.py:25-105)
        self.scene_dist, self.scene_grad = z(B, H, S), z(B, H, S, 4)
        self.cost, self.grad_q = z(B), z(B, H, self.action_dim)

    def update_env_query_idx(self, env_query_idx: Optional[torch.Tensor]) -> None:
        """Scene environment of every row (reference ``idxs_env`` / ``use_multi_env`` of the collision costs,
        cost/cost_scene_collision.py:58-198; batch-env planning, motion_planner_batch.py): row b collides with the obstacles of
        environment ``env_query_idx[b]``; ``None`` = every row uses env 0.  Switching between ``None`` and indices changes a
        kernel argument: re-capture graphs after it."""
        self.use_multi_env = env_query_idx is not None
        if env_query_idx is None:
            self.env_query_idx.zero_()
        else:
            validate_env_query_idx(env_query_idx, self.scene, self.kin.num_envs)
            self.env_query_idx.copy_(env_query_idx.to(device=self.device, dtype=torch.int32).reshape(-1))

    # ------------------------------------------------------------------ launches
    def _fk_forward(self, q: torch.Tensor, compute_com: bool = False) -> None:
        fk_forward_spheres(self.kin, self.link_pos, self.link_quat, self.robot_spheres, self.com, self.cumul_mat, q,
                           self.env_query_idx, self.batch_size * self._H, self._H, compute_com=compute_com)

    def _fk_backward(self, grad_pos, grad_quat, sphere_grad_a, sphere_grad_b, grad_com: Optional[torch.Tensor] = None) -> None:
        """grad_q <- the VJP of the tool-frame pose gradients and of the sum of the two sphere gradients (either may be None);
        ``grad_com`` [B, H, 4]: also of a centre-of-mass gradient (the forward must have run with ``compute_com``)"""
        k = self.kin
        kinematics_hip.launch_kinematics_backward(
            self.grad_q, grad_pos, grad_quat, sphere_grad_a, self.com if grad_com is None else grad_com, self.com, grad_pos,
            self.cumul_mat, k.link_spheres,
            k.link_masses_com, k.link_map, k.joint_map, k.joint_map_type, k.tool_frame_map, k.link_sphere_idx_map,
            k.link_chain_data, k.link_chain_offsets, k.joint_links_data, k.joint_links_offsets, k.joint_affects_endeffector,
            k.joint_offset_map, self.env_query_idx, k.num_envs, self.batch_size * self._H, self._H, self.action_dim,
            k.num_spheres if sphere_grad_a is not None else 0, grad_com is not None, False, grad_spheres_b=sphere_grad_b)

    def _self_collision(self, num_blocks_per_batch: int = 1, max_threads_per_block: int = 256) -> None:
        sc = self.kin.self_collision
        geometry_hip.self_collision_distance(
            self.self_dist, self.self_grad, self._pd, self.self_sparse, self.robot_spheres, sc.sphere_padding, self._w_self,
            sc.collision_pairs, self._bbmv, self._bbmi, num_blocks_per_batch, max_threads_per_block, self.batch_size, self._H,
            self.kin.num_spheres, sc.collision_pairs.shape[0], False, True)

    def _scene_collision(self, sweep: bool = False, speed_metric: bool = False, speed_dt: Optional[torch.Tensor] = None) -> None:
        collision_hip.sphere_obstacle_collision(
            self.scene_dist, self.scene_grad, self.robot_spheres, self.scene.struct, self._w_scene, self._eta_scene,
            self.env_query_idx, self.batch_size, self._H, self.kin.num_spheres, self.use_multi_env, 3 if sweep else 0,
            sweep and speed_metric, speed_dt)

    # ------------------------------------------------------------------ fused launch or kernel sequence
    @property
    def _use_self(self) -> bool:
        return True

    @property
    def _use_scene(self) -> bool:
        return self.scene is not None

    def _obstacle_slots(self) -> int:
        return obstacle_slots(self.scene) if self._use_scene else 0

    def _scene_has_meshes(self) -> bool:
        return self._use_scene and scene_has_meshes(self.scene)

    def _fused_fits(self, lds_bytes: int) -> bool:
        return not self._scene_has_meshes() and lds_bytes <= rollout_hip.FUSED_LDS_LIMIT and self.kin.num_links <= 128

    def _maybe_jit_shape(self) -> None:
        return None

    def _fused_chosen(self, veto: bool = False) -> bool:
        """the rollout's ``fused_available()`` (and no ``veto``), decided once per scene and batch size"""
        if self._fused_ok is None:
            self._fused_ok = self.fused_available() and not veto
            if self._fused_ok:
                self._maybe_jit_shape()
        return self._fused_ok


class BSplineRolloutBase(RobotRolloutBase):
    """Rows are B-spline trajectories: ``cfg.n_knots`` knots -> ``cfg.padded_horizon`` points from shared start / goal states."""

    #: the fused launch of this rollout carries the trajopt terms (pose, c-space): part of its compile-time shape
    with_trajopt_terms = False

    def __init__(self, kin, scene, cfg, self_collision_weight, scene_collision_weight, scene_activation_distance):
        super().__init__(kin, scene, cfg, self_collision_weight, scene_collision_weight, scene_activation_distance)
        self.action_horizon = cfg.n_knots
        d = self.device
        self._speed_dt, self._traj_dt = torch.tensor([cfg.traj_dt], device=d), torch.tensor([cfg.traj_dt], device=d)
        self._implicit_goal = torch.zeros(1, dtype=torch.uint8, device=d)

    def _alloc_bspline_buffers(self, B: int) -> None:
        """transition (reference StateFromBSplineKnot buffers, transition/fns_state_transition.py:310-472)"""
        z, H, D = self._zeros, self.cfg.padded_horizon, self.action_dim
        self.position, self.velocity, self.acceleration, self.jerk = z(B, H, D), z(B, H, D), z(B, H, D), z(B, H, D)
        self.out_dt = z(B)
        self.start_idx, self.goal_idx = z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.grad_knots = z(B, self.cfg.n_knots, D)

    def update_start_state(self, start_position: Optional[torch.Tensor], start_velocity: Optional[torch.Tensor] = None,
                           start_acceleration: Optional[torch.Tensor] = None, start_idx: Optional[torch.Tensor] = None) -> None:
        """Start state(s) of the trajectories: position [n, D] (+ velocity / acceleration for a robot in motion: the
        B-spline's fixed knots reproduce them, bspline_boundary_constraint.cuh:330-367); ``start_idx`` [B] picks the
        start state of every trajectory (reference ``idxs_start``; default: state 0)."""
        D, d = self.action_dim, self.device
        if start_position is None:
            start_position = torch.zeros(1, D, device=d)
        sp = start_position.to(d, torch.float32).reshape(-1, D).contiguous()
        if start_idx is not None:
            self.start_idx.copy_(start_idx.to(device=d, dtype=torch.int32).reshape(-1))
        if getattr(self, "start_pos", None) is not None and self.start_pos.shape == sp.shape:
            self.start_pos.copy_(sp)  # keep the pointers a captured hipGraph holds
            self.start_vel.copy_(start_velocity.to(d, torch.float32).reshape(-1, D)) if start_velocity is not None else self.start_vel.zero_()
            self.start_acc.copy_(start_acceleration.to(d, torch.float32).reshape(-1, D)) if start_acceleration is not None else self.start_acc.zero_()
            return
        self.start_pos = sp.clone()
        n = self.start_pos.shape[0]
        self.start_vel, self.start_acc, self.start_jerk = (torch.zeros(n, D, device=d) for _ in range(3))
        if start_velocity is not None:
            self.start_vel.copy_(start_velocity.to(d, torch.float32).reshape(-1, D))
        if start_acceleration is not None:
            self.start_acc.copy_(start_acceleration.to(d, torch.float32).reshape(-1, D))
        if getattr(self, "goal_pos", None) is None:
            self.goal_pos, self.goal_vel, self.goal_acc, self.goal_jerk = (torch.zeros(1, D, device=d) for _ in range(4))

    def _bspline_args(self):
        """the start / goal states and per-trajectory indices every B-spline launch (the fused ones included) takes, in order"""
        return (self.start_pos, self.start_vel, self.start_acc, self.start_jerk, self.goal_pos, self.goal_vel, self.goal_acc,
                self.goal_jerk, self.start_idx, self.goal_idx, self._traj_dt, self._implicit_goal)

    def _bspline_forward(self, act_seq: torch.Tensor) -> None:
        """knots -> position / velocity / acceleration / jerk buffers (reference ``compute_state_from_action``)"""
        c = self.cfg
        trajectory_hip.launch_bspline_interpolation_forward_kernel(
            self.position, self.velocity, self.acceleration, self.jerk, self.out_dt, act_seq, *self._bspline_args(),
            self.batch_size, c.padded_horizon, self.action_dim, c.n_knots, c.bspline_degree)

    def _bspline_backward(self, grad_v, grad_a, grad_j) -> None:
        """grad_knots <- the VJP of grad_q and of the velocity / acceleration / jerk gradients"""
        c = self.cfg
        trajectory_hip.launch_bspline_interpolation_backward_kernel(
            self.grad_knots, self.grad_q, grad_v, grad_a, grad_j, self._traj_dt, self.goal_idx, self._implicit_goal,
            self.batch_size, c.padded_horizon, self.action_dim, c.n_knots, c.bspline_degree, False)

    def _maybe_jit_shape(self) -> None:
        """cfg.jit_shape / CUROBO_HIP_JIT_SHAPES: a compile-time shape for this rollout's dimensions, built once when the library
        has none (never inside a captured launch sequence: the first call of a rollout is an eager warm-up)"""
        from ..backends import fused_jit

        if not (self.cfg.jit_shape or fused_jit.enabled_by_env()) or not self._use_self:
            return
        k, c = self.kin, self.cfg
        lanes = getattr(k.self_collision.collision_pairs, "_self_lane_lists", None)
        fused_jit.ensure_shape(c.padded_horizon, c.n_knots, self.action_dim, k.num_links, k.num_spheres,
                               int(k.self_collision.collision_pairs.shape[0]), int(k.link_chain_data.shape[0]),
                               int(lanes[1]) if lanes is not None else 0, self._obstacle_slots(),
                               with_trajopt_terms=self.with_trajopt_terms)

    def _dispatch_order(self):
        """longest-first dispatch workspace of this rollout's fused launches (cfg.longest_first_dispatch)"""
        if not self.cfg.longest_first_dispatch:
            return None
        if self._dispatch is None:
            self._dispatch = rollout_hip.DispatchOrder(self.batch_size, self.cost.device)
        return self._dispatch

    # ------------------------------------------------------------------ reuse of evaluations the caller holds
    def _reuse_row_arrays(self):
        """everything a launch reads PER TRAJECTORY besides the knots (the launch's ``memo`` compares only those)"""
        return [self.start_idx, self.goal_idx, self.env_query_idx]

    def _reuse_launch_ok(self) -> bool:
        """``cost_and_gradient`` is the fused launch and materialises nothing (a copied row cannot fill such outputs)"""
        return False

    def offers_reuse(self, stride: int) -> bool:
        """Whether ``cost_and_gradient(x, memo=(x_held, cost, grad, stride))`` may serve row ``stride * i`` from held row ``i``
        (an optimiser: the line-search candidate with step 0 from the exploration point it kept).  A held row is the result of
        ANOTHER row of the same group of ``stride`` rows, evaluated one launch earlier, so the per-trajectory arrays must be
        equal within every group: the rollouts fill them by repetition per problem, and that is checked here (one read-back,
        cached until one of the arrays is written again; never under graph capture, where an unchecked state means no reuse).
        What the check cannot see is the caller's contract: scene, weights and the start / goal rows themselves stay as
        they are between the evaluation that produced a held row and the launch that reuses it."""
        B = self.batch_size
        if stride < 1 or B == 0 or B % stride != 0 or not self._reuse_launch_ok():
            return False
        arrays = self._reuse_row_arrays()
        key = (stride, B, tuple((t.data_ptr(), t._version) for t in arrays))
        if getattr(self, "_reuse_key", None) != key:
            if torch.cuda.is_current_stream_capturing():
                return False
            groups = [t.reshape(B // stride, stride, -1) for t in arrays]
            self._reuse_uniform = all(bool((g == g[:, :1]).all()) for g in groups)
            self._reuse_key = key
        return self._reuse_uniform

    def _checked_memo(self, memo):
        """``memo`` as the launch takes it; a memo this rollout cannot honour is an error, not an evaluation in full"""
        if memo is not None and not self.offers_reuse(int(memo[3])):
            raise ValueError("memo: this rollout offers no reuse at this stride (offers_reuse): kernel sequence, materialised "
                             "outputs, or per-trajectory arrays that differ within a group of rows")
        return memo


class PoseTerms:
    """The tool-pose goal term of a rollout (mixin): goal sets per row, per-frame weight factors / tolerances, one launch."""

    def _init_pose_terms(self, pose_weight, convergence_tolerance, non_terminal_factor: Optional[float]) -> None:
        """``non_terminal_factor`` None = a rollout of one point per row: its terminal rows serve as the non-terminal ones too"""
        d, T = self.device, self.kin.num_pose_links
        self._pose_w = torch.tensor(pose_weight, device=d, dtype=torch.float32)
        self._axes_w = torch.ones(T, 6, device=d)
        self._tol = torch.tensor([convergence_tolerance] * T, device=d, dtype=torch.float32)
        self._project = torch.zeros(T, dtype=torch.uint8, device=d)
        if non_terminal_factor is None:
            self._axes_w0, self._tol0 = self._axes_w, self._tol
        else:
            self._axes_w0, self._tol0 = torch.full((T, 6), float(non_terminal_factor), device=d), self._tol.clone()

    def _alloc_pose_buffers(self, B: int, H: int, num_goalset: int) -> None:
        z, T = self._zeros, self.kin.num_pose_links
        self.pose_cost, self.pose_pos_dist, self.pose_rot_dist = z(B, H, 2 * T), z(B, H, T), z(B, H, T)
        self.pose_grad_pos, self.pose_grad_quat = z(B, H, T, 3), z(B, H, T, 4)
        self.goalset_idx = z(B, H, T, dt=torch.int32)
        self.idxs_goal, self._idx0 = z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.goal_position, self.goal_quat = z(1, T, num_goalset, 3), z(1, T, num_goalset, 4)
        self.goal_quat[..., 0] = 1.0

    def _update_goal_poses(self, goal_position: torch.Tensor, goal_quat: torch.Tensor) -> bool:
        """in place when the shape is unchanged (captured graphs hold the pointers); True = new buffers: re-capture"""
        if goal_position.shape == self.goal_position.shape:
            self.goal_position.copy_(goal_position)
            self.goal_quat.copy_(goal_quat)
            return False
        self.goal_position = goal_position.to(self.device, torch.float32).contiguous().clone()
        self.goal_quat = goal_quat.to(self.device, torch.float32).contiguous().clone()
        return True

    def update_tool_pose_criteria(self, criteria) -> None:
        """``{tool frame: ToolPoseCriteria}`` -> the per-frame factor / tolerance / projection rows the pose cost reads
        (reference ToolPoseCost.update_tool_pose_criteria); written in place, so captured graphs see the new values"""
        for name, c in criteria.items():
            if name not in self.kin.tool_frames:
                raise ValueError(f"tool frame {name} not in {self.kin.tool_frames}")
            i, f = self.kin.tool_frames.index(name), lambda v: torch.tensor(v, device=self.device, dtype=torch.float32)  # noqa: E731
            non_terminal = self._axes_w0 is not self._axes_w
            self._axes_w[i].copy_(f(c.terminal_pose_axes_weight_factor))
            if non_terminal:
                self._axes_w0[i].copy_(f(c.non_terminal_pose_axes_weight_factor))
            self._tol[i].copy_(f(c.terminal_pose_convergence_tolerance))
            if non_terminal:
                self._tol0[i].copy_(f(c.non_terminal_pose_convergence_tolerance))
            self._project[i] = int(bool(c.project_distance_to_goal))

    def _pose_term(self) -> None:
        cost_hip.tool_pose_distance(
            self.pose_cost, self.pose_pos_dist, self.pose_rot_dist, self.pose_grad_pos, self.pose_grad_quat, self.goalset_idx,
            self.link_pos, self.link_quat, self.goal_position, self.goal_quat, self.idxs_goal, self._pose_w, self._axes_w,
            self._axes_w0, self._tol, self._tol0, self._project, self.batch_size, self._H, self.kin.num_pose_links,
            int(self.goal_position.shape[2]), self.cfg.rotation_method)
