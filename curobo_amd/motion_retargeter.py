"""``MotionRetargeter``: a clip of per-frame tool-pose targets -> a joint trajectory (reference ``curobo.motion_retargeter``:
``_src/motion/motion_retargeter.py:56-404``, ``motion_retargeter_cfg.py:16-210``, ``motion_retargeter_result.py``).

The first frame is solved with global IK (many seeds); every later frame with IK seeded at the previous solution and held to what
the joints can do in ``optimization_dt`` from it (``InverseKinematicsCfg.optimization_dt``: velocity-tightened joint limits and the
implied velocity / acceleration regularisation in every rollout, ``curobo_hip_rollout_ik_fused_state``).  The MPC mode of the
reference (``use_mpc=True``) is not built.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Union

import torch

from .kinematics import Kinematics
from .optim import LBFGSOptCfg
from .rollout.ik_rollout import IKRolloutCfg
from .solver.ik import IKSolverCfg
from .solver.inverse_kinematics import InverseKinematics, InverseKinematicsCfg
from .types import DeviceCfg, GoalToolPose, JointState, SequenceGoalToolPose, ToolPoseCriteria


def retarget_ik_task_cfg() -> IKSolverCfg:
    """the cost and optimiser values of the reference's ``content/configs/task/ik/lbfgs_retarget_ik.yml``, for both IK solvers"""
    return IKSolverCfg(
        rollout=IKRolloutCfg(pose_weight=[1000.0, 100.0], pose_convergence_tolerance=[1e-8, 1e-8], cspace_weight=[10000.0, 0.0],
                             cspace_activation_distance=[0.01, 0.01], scene_collision_weight=10000.0, scene_activation_distance=0.0,
                             self_collision_weight=10000.0, squared_l2_regularization_weight=[0.01, 0.01]),
        optimizer=LBFGSOptCfg(history=15, inner_iters=20, num_iters=200, cost_relative_threshold=0.01, fixed_iters=True))


@dataclass
class MotionRetargeterCfg:
    """fields, defaults and ``create`` of the reference's MotionRetargeterCfg (motion_retargeter_cfg.py:30-200)"""

    #: packaged robot name / robot yaml path / its dictionary
    robot: Union[str, Dict[str, Any]]
    #: ``{tool frame: ToolPoseCriteria}``: weights of the position (xyz) and rotation (rpy) terms per tracked frame
    tool_pose_criteria: Dict[str, ToolPoseCriteria]
    #: clips retargeted in parallel
    num_envs: int = 1
    #: MPC for frames 1+ (not built: raises NotImplementedError when a retargeter is made)
    use_mpc: bool = False
    self_collision_check: bool = True
    scene_model: Optional[Union[str, Dict[str, Any]]] = None
    #: time step [s] of the velocity-limited IK
    optimization_dt: float = 0.05
    #: seeds of the first frame's global IK
    num_seeds_global: int = 64
    position_tolerance: float = 0.005
    orientation_tolerance: float = 0.05
    device_cfg: DeviceCfg = field(default_factory=DeviceCfg)
    #: switched off when neither self collision nor a scene needs the spheres
    load_collision_spheres: bool = True
    #: accepted and ignored: the values of ``ik/lbfgs_retarget_ik.yml`` are built in (``retarget_ik_task_cfg``)
    ik_optimizer_configs: List[Union[str, Dict[str, Any]]] = field(default_factory=lambda: ["ik/lbfgs_retarget_ik.yml"])
    #: accepted and ignored (MPC mode)
    mpc_optimizer_configs: List[Union[str, Dict[str, Any]]] = field(default_factory=lambda: ["mpc/lbfgs_retarget_mpc.yml"])
    #: seeds of the warm-started IK of frames 1+
    num_seeds_local: int = 1
    num_control_points: Optional[int] = None
    steps_per_target: int = 8
    #: weight on (q - q_prev) / dt; None = the task value (0.01)
    velocity_regularization_weight: Optional[float] = None
    #: weight on (v - v_prev) / dt; None = the task value (0.01)
    acceleration_regularization_weight: Optional[float] = None
    collision_activation_distance: float = 0.01
    #: L-BFGS iterations of the first frame / of frames 1+; None = the task value (200)
    global_ik_num_iters: Optional[int] = None
    local_ik_num_iters: Optional[int] = None
    mpc_warm_start_num_iters: int = 100
    mpc_cold_start_num_iters: int = 300
    #: the support-polygon (balance) term of both IK solvers (``InverseKinematicsCfg``): None = off.  Fields of this dataclass
    #: only (``dataclasses.replace(MotionRetargeterCfg.create(...), support_polygon_weight=..., foot_link_names=[...])``):
    #: ``create`` keeps the reference's argument list
    support_polygon_weight: Optional[float] = None
    foot_link_names: Optional[List[str]] = None

    @property
    def tool_frames(self) -> List[str]:
        return list(self.tool_pose_criteria.keys())

    @staticmethod
    def create(robot: Union[str, Dict[str, Any]], tool_pose_criteria: Dict[str, ToolPoseCriteria], num_envs: int = 1,
               use_mpc: bool = False, self_collision_check: bool = True, scene_model: Optional[Union[str, Dict[str, Any]]] = None,
               optimization_dt: float = 0.05, num_seeds_global: int = 64, load_collision_spheres: bool = True,
               ik_optimizer_configs: Optional[List[Union[str, Dict[str, Any]]]] = None,
               mpc_optimizer_configs: Optional[List[Union[str, Dict[str, Any]]]] = None, num_seeds_local: int = 1,
               num_control_points: Optional[int] = 12, steps_per_target: int = 4, position_tolerance: float = 0.005,
               orientation_tolerance: float = 0.05, device_cfg: Optional[DeviceCfg] = None,
               velocity_regularization_weight: Optional[float] = None, acceleration_regularization_weight: Optional[float] = None,
               collision_activation_distance: float = 0.01, global_ik_num_iters: Optional[int] = None,
               local_ik_num_iters: Optional[int] = None, mpc_warm_start_num_iters: int = 100,
               mpc_cold_start_num_iters: int = 300) -> "MotionRetargeterCfg":
        return MotionRetargeterCfg(
            robot=robot, tool_pose_criteria=tool_pose_criteria, num_envs=num_envs, use_mpc=use_mpc,
            self_collision_check=self_collision_check, scene_model=scene_model, optimization_dt=optimization_dt,
            num_seeds_global=num_seeds_global, load_collision_spheres=load_collision_spheres,
            ik_optimizer_configs=ik_optimizer_configs if ik_optimizer_configs is not None else ["ik/lbfgs_retarget_ik.yml"],
            mpc_optimizer_configs=mpc_optimizer_configs if mpc_optimizer_configs is not None else ["mpc/lbfgs_retarget_mpc.yml"],
            num_seeds_local=num_seeds_local, num_control_points=num_control_points, steps_per_target=steps_per_target,
            position_tolerance=position_tolerance, orientation_tolerance=orientation_tolerance,
            device_cfg=device_cfg if device_cfg is not None else DeviceCfg(),
            velocity_regularization_weight=velocity_regularization_weight,
            acceleration_regularization_weight=acceleration_regularization_weight,
            collision_activation_distance=collision_activation_distance, global_ik_num_iters=global_ik_num_iters,
            local_ik_num_iters=local_ik_num_iters, mpc_warm_start_num_iters=mpc_warm_start_num_iters,
            mpc_cold_start_num_iters=mpc_cold_start_num_iters)

    def __post_init__(self):
        if not self.self_collision_check and self.scene_model is None:
            self.load_collision_spheres = False
        if self.self_collision_check and not self.load_collision_spheres:
            raise ValueError("load_collision_spheres must be True when self_collision_check is True")
        if self.scene_model is not None and not self.load_collision_spheres:
            raise ValueError("load_collision_spheres must be True when scene_model is not None")


@dataclass
class RetargetResult:
    """``solve_frame``: joint_state [num_envs, dof]; ``solve_sequence``: [num_envs, frames, dof] (reference RetargetResult)"""

    joint_state: JointState
    #: the intermediate MPC trajectory (MPC mode only)
    trajectory: Optional[JointState] = None
    #: whether the frame's IK reported success: [num_envs] per frame, [num_envs, frames] for a sequence (this package's field)
    success: Optional[torch.Tensor] = None


class MotionRetargeter:
    """Keeps the previous solution between calls of ``solve_frame``: the first call is global IK, the following ones are
    warm-started and velocity-limited; ``reset`` starts a new clip."""

    def __init__(self, config: MotionRetargeterCfg):
        if config.use_mpc:
            raise NotImplementedError("MotionRetargeterCfg.use_mpc=True: MPC-mode retargeting is not built (the IK mode, "
                                      "use_mpc=False, is)")
        self._config = config
        self._num_envs = config.num_envs
        self._tool_pose_criteria = config.tool_pose_criteria
        self._global_ik_solver = self._build_ik_solver(local=False)
        self._local_ik_solver = self._build_ik_solver(local=True)
        self._joint_names = list(self._global_ik_solver.joint_names)
        self._action_dim = self._global_ik_solver.action_dim
        self._prev_solution: Optional[torch.Tensor] = None
        self._prev_velocity: Optional[torch.Tensor] = None

    def _build_ik_solver(self, local: bool) -> InverseKinematics:
        """frame 0: global search, no velocity limit; frames 1+: seeded at the previous solution, one time step from it
        (reference _build_global_ik_solver / _build_local_ik_solver, motion_retargeter.py:336-384)"""
        c = self._config
        kw = dict(num_seeds=c.num_seeds_global, optimization_dt=None,
                  override_optimizer_num_iters={"lbfgs": c.global_ik_num_iters})
        if local:
            kw = dict(num_seeds=c.num_seeds_local, optimization_dt=c.optimization_dt,
                      override_optimizer_num_iters={"lbfgs": c.local_ik_num_iters},
                      velocity_regularization_weight=c.velocity_regularization_weight,
                      acceleration_regularization_weight=c.acceleration_regularization_weight, use_lm_seed=False, exit_early=False)
        ik_cfg = InverseKinematicsCfg.create(
            robot=c.robot, position_tolerance=c.position_tolerance, orientation_tolerance=c.orientation_tolerance,
            self_collision_check=c.self_collision_check, scene_model=c.scene_model, override_iters_for_multi_link_ik=None,
            optimizer_configs=c.ik_optimizer_configs, device_cfg=c.device_cfg, load_collision_spheres=c.load_collision_spheres,
            optimizer_collision_activation_distance=c.collision_activation_distance, max_batch_size=c.num_envs,
            support_polygon_weight=c.support_polygon_weight, foot_link_names=c.foot_link_names, **kw)
        ik_cfg.task_cfg = retarget_ik_task_cfg()
        solver = InverseKinematics(ik_cfg)
        solver.update_tool_pose_criteria(self._tool_pose_criteria)
        return solver

    # ------------------------------------------------------------------ reference members
    @property
    def joint_names(self) -> List[str]:
        return self._joint_names

    @property
    def action_dim(self) -> int:
        return self._global_ik_solver.action_dim

    @property
    def num_dof(self) -> int:
        """deprecated alias of ``action_dim``"""
        return self.action_dim

    @property
    def tool_frames(self) -> List[str]:
        return self._global_ik_solver.tool_frames

    @property
    def kinematics(self) -> Kinematics:
        return self._global_ik_solver.kinematics

    @property
    def default_joint_state(self) -> JointState:
        return self._global_ik_solver.default_joint_state

    @property
    def config(self) -> MotionRetargeterCfg:
        return self._config

    def reset(self) -> None:
        """forget the previous solution: the next ``solve_frame`` is global IK, from the seeds the first one started from (the
        seed stage's sample stream is rewound, so the same clip gives the same trajectory again)"""
        self._prev_solution = None
        self._prev_velocity = None
        self._global_ik_solver.reset_seed()

    def solve_frame(self, goal_tool_poses: GoalToolPose) -> RetargetResult:
        """goal poses [num_envs, 1, num_links, num_goalset, 3 | 4] of the robot's tool frames -> joint_state [num_envs, dof]"""
        if goal_tool_poses.batch_size != self._num_envs:
            raise ValueError(f"GoalToolPose batch size ({goal_tool_poses.batch_size}) does not match num_envs ({self._num_envs}) "
                             "from config")
        if self._prev_solution is None:
            return self._solve_global_ik(goal_tool_poses)
        return self._solve_local_ik(goal_tool_poses)

    def solve_sequence(self, tool_poses: SequenceGoalToolPose) -> RetargetResult:
        """a clip [num_frames, num_envs, num_links, num_goalset, 3 | 4] -> joint_state [num_envs, num_frames, dof], from a reset"""
        if tool_poses.num_envs != self._num_envs:
            raise ValueError(f"SequenceGoalToolPose num_envs ({tool_poses.num_envs}) does not match num_envs ({self._num_envs}) "
                             "from config")
        self.reset()
        frames = [self.solve_frame(tool_poses.get_frame(t)) for t in range(tool_poses.num_frames)]
        stack = lambda f: (torch.stack([getattr(r.joint_state, f) for r in frames], dim=1)  # noqa: E731
                           if getattr(frames[0].joint_state, f) is not None else None)
        js = JointState(position=stack("position"), velocity=stack("velocity"), acceleration=stack("acceleration"),
                        joint_names=self._joint_names)
        return RetargetResult(joint_state=js, trajectory=None, success=torch.stack([r.success for r in frames], dim=1))

    def _solve_global_ik(self, goal_tool_poses: GoalToolPose) -> RetargetResult:
        result = self._global_ik_solver.solve_pose(goal_tool_poses=goal_tool_poses, return_seeds=1)
        sol = result.js_solution.position.view(self._num_envs, self._action_dim)
        self._prev_solution = sol.clone()
        return RetargetResult(joint_state=JointState.from_position(sol, joint_names=self._joint_names),
                              success=result.success.view(self._num_envs))

    def _solve_local_ik(self, goal_tool_poses: GoalToolPose) -> RetargetResult:
        n, D = self._num_envs, self._action_dim
        seed = self._prev_solution.view(n, 1, D).expand(n, self._config.num_seeds_local, D)
        current_state = JointState.from_position(self._prev_solution.clone(), joint_names=self._joint_names)
        if self._prev_velocity is not None:
            current_state.velocity = self._prev_velocity.clone()
        result = self._local_ik_solver.solve_pose(goal_tool_poses=goal_tool_poses, seed_config=seed, current_state=current_state,
                                                  return_seeds=1)
        sol = result.js_solution.position.view(n, D)
        if result.js_solution.velocity is not None:
            self._prev_velocity = result.js_solution.velocity.view(n, D)
        self._prev_solution = sol.clone()
        return RetargetResult(joint_state=JointState.from_position(sol, joint_names=self._joint_names),
                              success=result.success.view(n))
