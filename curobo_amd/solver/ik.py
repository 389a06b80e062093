"""Batched collision-free inverse kinematics: many random seeds per goal pose, L-BFGS on every
seed in parallel, best successful seed per problem.

Mirrors the flow of the reference ``IKSolver._solve_impl`` (``curobo/_src/solver/solver_ik.py:363-586``):
seeds -> ``optimizer.optimize`` -> metrics rollout -> success mask -> ``cost + 1e16 * fail`` ->
top-1 over seeds.  Seeds come from the Levenberg-Marquardt seed solver (``use_lm_seed``, reference
``solver_ik.py:707-722``: the best ``num_seeds`` of ``seed_solver_num_seeds`` LM runs) or are uniform
within the joint limits.  ``stream_shards`` > 1 splits the problems over L-BFGS instances on their own
HIP streams inside one graph (``optim/pipelined.py``).  With ``torch.distributed`` initialised the seed axis is sharded and the
winner found with one RCCL all-gather (``curobo_amd.distributed.global_argmin``).
"""

from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Optional

import torch

from ..distributed import global_argmin, global_topk, shard_range
from ..optim import LBFGSOpt, LBFGSOptCfg, PipelinedLBFGS
from ..robot.kinematics_params import KinematicsParams
from ..rollout.ik_rollout import IKRollout, IKRolloutCfg
from ..scene.data import SceneData
from ..util.graph_capture import capture_graph
from .seed_ik import SeedIKSolver, SeedIKSolverCfg


@dataclass
class IKSolverCfg:
    num_seeds: int = 64
    position_threshold: float = 0.005  # reference solver_ik defaults
    rotation_threshold: float = 0.05
    rollout: IKRolloutCfg = field(default_factory=IKRolloutCfg)
    # optimizer: content/configs/task/ik/lbfgs_ik.yml:38-70
    optimizer: LBFGSOptCfg = field(default_factory=lambda: LBFGSOptCfg(
        history=7, inner_iters=20, num_iters=100, cost_relative_threshold=0.01))
    seed: int = 0
    #: seeds of the optimiser = best ``num_seeds`` solutions of the LM seed solver (reference
    #: solver_ik_cfg.py:71,93; solver_ik.py:131-141: at least 2 x num_seeds LM runs)
    use_lm_seed: bool = True
    seed_solver_num_seeds: int = 32
    #: problem shards of the optimiser on separate HIP streams (1 = one batch, one stream)
    stream_shards: int = 1
    #: alternative goal poses per problem (reference IKSolverCfg.max_goalset): a solution may reach any one
    num_goalset: int = 1
    #: reference IKSolverCfg.exit_early / exit_early_batch_success_threshold (solver_ik_cfg.py:74-77,
    #: solver_ik.py:395-404): when the seed-IK solutions already pass every check (pose error, joint
    #: limits, self and scene collision) for at least this fraction of the problems, they are returned
    #: and the L-BFGS stage is skipped.  Costs one device->host read of the success count, as there.
    exit_early: bool = True
    exit_early_batch_success_threshold: float = 1.0
    #: reference IKSolverCfg.override_iters_for_multi_link_ik (solver_ik_cfg.py:68, solver_ik.py:115-128): the L-BFGS iteration
    #: count is raised to this when it is lower (its benchmark sets 240 for the Unitree G1)
    override_iters_for_multi_link_ik: Optional[int] = None
    #: with ``solve_pose(current_position=)`` the solutions are ranked as the reference ranks them (solver_ik.py:463-500): by the sum
    #: of the position [m] and rotation [rad] errors over the tool frames + this weight x 0.5 |q - current|^2 (its ``start_cspace_dist``
    #: convergence metric, metrics_base.yml:27-30: weight 0.001), so that among the solutions that succeed the ones near the robot's
    #: configuration come first unless they are millimetres less accurate.  Without a current position: the rollout's cost, as before.
    start_cspace_dist_weight: float = 0.001
    #: reference IKSolverCfg.optimization_dt (solver_ik_cfg.py:159-162): the time step [s] in which a solution has to be reachable
    #: from ``solve_pose(current_position=)``.  Set: every rollout -- the metrics rollout too, as the reference hands one goal with
    #: ``current_js`` / ``current_state_dt`` to all of them (cost_manager_robot.py:250-256) -- carries the current state: the joint
    #: limits are tightened to ``current +- velocity_limits * dt``, ``rollout.squared_l2_regularization_weight`` regularises the
    #: implied velocity / acceleration, and ``success`` requires a solution within one step.  None: no current state anywhere.
    optimization_dt: Optional[float] = None


@dataclass
class IKResult:
    success: torch.Tensor  # [P] bool
    solution: torch.Tensor  # [P, D]
    position_error: torch.Tensor  # [P]
    rotation_error: torch.Tensor  # [P]
    cost: torch.Tensor  # [P]
    seed_index: torch.Tensor  # [P] global seed index of the winner
    goalset_index: Optional[torch.Tensor] = None  # [P, T] member of the goal set the solution reaches, per tool frame
    #: [P] signed distance [m] of the solution's centre of mass (xy) to its support polygon, negative inside; None when the
    #: support-polygon term is off (``rollout.support_polygon_weight`` = 0)
    support_polygon_distance: Optional[torch.Tensor] = None


class IKSolver:
    def __init__(self, kin: KinematicsParams, scene: Optional[SceneData], num_problems: int,
                 cfg: Optional[IKSolverCfg] = None, seed_offset: int = 0, use_cuda_graph: bool = True,
                 global_num_seeds: Optional[int] = None):
        """``cfg.num_seeds`` seeds per problem run in this process: seeds ``[seed_offset, seed_offset + num_seeds)`` of
        ``global_num_seeds`` when the seed axis is sharded over ranks (default: all of them; ``IKSolver.sharded``
        derives the shard of this rank from ``torch.distributed``)."""
        self.kin, self.scene, self.cfg = kin, scene, cfg or IKSolverCfg()
        from ..scene.data import warn_if_reference_mesh_gradient

        warn_if_reference_mesh_gradient(scene, "IKSolver")
        self._use_graph, self._result_graphs = use_cuda_graph, {}
        self.P, self.S = num_problems, self.cfg.num_seeds
        self.device = kin.device
        self.seed_offset = seed_offset
        self.S_global = int(global_num_seeds) if global_num_seeds is not None else self.S
        # private copy of the optimiser configuration: the caller's cfg may be shared by solvers of other sizes
        ocfg = dataclasses.replace(self.cfg.optimizer, num_problems=self.P * self.S)
        if self.cfg.override_iters_for_multi_link_ik is not None and ocfg.num_iters < int(self.cfg.override_iters_for_multi_link_ik):
            inner = max(int(ocfg.inner_iters), 1)
            ocfg = dataclasses.replace(ocfg, num_iters=-(-int(self.cfg.override_iters_for_multi_link_ik) // inner) * inner)
        self.cfg = dataclasses.replace(self.cfg, optimizer=ocfg)
        self.nls = len(ocfg.line_search_scale)
        self.G = self.cfg.num_goalset
        # the metrics rollout decides feasibility as the reference's does (content/configs/task/metrics_base.yml:8-19): joint limits
        # and scene collision at ZERO activation distance -- a solution inside the optimiser's 0.01 rad / 2.5 mm activation shells
        # is inside the limits and clear of the world (with 49 joints a quarter of the G1's solutions sit within 0.01 rad of a limit)
        # with a current state: the same position term at zero activation and zero regularisation (cost_cspace_cfg.py:84-119)
        self._with_state = self.cfg.optimization_dt is not None
        self.metrics_rollout = IKRollout(kin, scene, self.P * self.S, dataclasses.replace(
            self.cfg.rollout, cspace_activation_distance=[0.0] * len(self.cfg.rollout.cspace_activation_distance),
            scene_activation_distance=0.0, squared_l2_regularization_weight=[0.0, 0.0]), num_goalset=self.G,
            use_current_state=self._with_state)
        bounds = (kin.joint_limits_position[0], kin.joint_limits_position[1])
        K = self.cfg.stream_shards
        if K > 1 and self.P % K != 0:
            raise ValueError(f"num_problems ({self.P}) must be a multiple of stream_shards ({K})")
        rows_per_problem = self.S * self.nls
        self.rollouts = []

        def make_rollout(batch, k=0):
            ro = IKRollout(kin, scene, batch, self.cfg.rollout, num_goalset=self.G, use_current_state=self._with_state)
            ro._first_problem = k * (self.P // K)  # rows of shard k belong to problems [first, first + P/K)
            self.rollouts.append(ro)
            return ro.cost_and_gradient
        if K > 1:
            self.optimizer = PipelinedLBFGS(ocfg, make_rollout, 1, kin.num_dof, bounds, self.device, n_shards=K,
                                            use_cuda_graph=use_cuda_graph)
        else:
            self.optimizer = LBFGSOpt(ocfg, make_rollout(self.P * rows_per_problem), 1, kin.num_dof, bounds, self.device,
                                      use_cuda_graph=use_cuda_graph)
        for o in getattr(self.optimizer, "opts", [self.optimizer]):
            o.rank_sharded = self.S_global != self.S  # the seed axis is split over ranks: the convergence exit is a collective
        self.rollout = self.rollouts[0]
        self._row_goals = [(ro._first_problem + torch.arange(ro.batch_size, device=self.device) // rows_per_problem).to(torch.int32)
                           for ro in self.rollouts]
        self._mrow_goal = (torch.arange(self.P * self.S, device=self.device) // self.S).to(torch.int32)
        self.seed_solver = None
        if self.cfg.use_lm_seed:
            # the LM seed stage works on ONE global Halton set whatever the world size (W = 1 and
            # W = 8 draw the same seeds): max(seed_solver_num_seeds, 2 x global seeds) LM runs per problem, this rank
            # takes a contiguous slice of them, all ranks rank them together and the optimiser seeds of this rank are
            # rows [seed_offset, seed_offset + num_seeds) of that ranking
            # robots with several tool frames get more and longer LM runs, as the reference's IKSolver sets them
            # (solver_ik.py:109-141: 128 runs x 20 iterations for two frames, 64 x 30 for more; 16 iterations otherwise)
            n_frames = len(kin.tool_frames) if getattr(kin, "tool_frames", None) is not None else 1
            lm_runs, lm_iters, lm_inner = self.cfg.seed_solver_num_seeds, 16, 4
            if n_frames > 1:
                lm_runs, lm_iters, lm_inner = 128, 20, 4
            if n_frames > 2:
                lm_runs, lm_iters, lm_inner = 64, 30, 5
            n_lm = max(lm_runs, 2 * self.S_global)
            lm_lo, lm_hi = 0, n_lm
            if self.S_global != self.S:
                import torch.distributed as dist

                if not (dist.is_available() and dist.is_initialized()):
                    raise ValueError("a seed shard (global_num_seeds != num_seeds) needs torch.distributed initialised")
                rank, world = dist.get_rank(), dist.get_world_size()
                if shard_range(self.S_global, rank, world) != (seed_offset, seed_offset + self.S):
                    raise ValueError(f"seed shard [{seed_offset}, {seed_offset + self.S}) of {self.S_global} is not rank {rank}'s "
                                     f"contiguous shard {shard_range(self.S_global, rank, world)} (world size {world})")
                lm_lo, lm_hi = shard_range(n_lm, rank, world)
            self.seed_solver = SeedIKSolver(kin, self.P, SeedIKSolverCfg(num_seeds=lm_hi - lm_lo, use_cuda_graph=use_cuda_graph,
                                                                         sampler_seed=451 + self.cfg.seed, max_iterations=lm_iters,
                                                                         inner_iterations=lm_inner, lambda_initial=1.0, rho_min=1e-5),
                                            num_goalset=self.G, seed_offset=lm_lo, global_num_seeds=n_lm)
            # one set of goal buffers for the metrics rollout and the seed stage ([P, T, G, 3 | 4] both): a solve uploads
            # its goals once (shared BEFORE anything is captured: the graphs hold these addresses)
            self.metrics_rollout.goal_position, self.metrics_rollout.goal_quat = self.seed_solver.goal_position, self.seed_solver.goal_quat
        self._gen = torch.Generator(device="cpu")
        # the robot's configuration and the weight of its distance term in the ranking: fixed buffers (the ranking is a captured graph)
        self._cur_buf = torch.zeros(self.P, kin.num_dof, device=self.device)
        self._cur_w = torch.zeros(1, device=self.device)
        self._set_current_state(None, None, None)  # (the state buffers get their size before anything is captured)

    @classmethod
    def sharded(cls, kin: KinematicsParams, scene: Optional[SceneData], num_problems: int, cfg: Optional[IKSolverCfg] = None,
                use_cuda_graph: bool = True) -> "IKSolver":
        """``cfg.num_seeds`` is the GLOBAL seed count; the solver of this rank runs its contiguous shard of it
        (``distributed.shard_range``).  Alone in the process this is the plain solver."""
        import torch.distributed as dist

        cfg = cfg or IKSolverCfg()
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return cls(kin, scene, num_problems, cfg, use_cuda_graph=use_cuda_graph)
        lo, hi = shard_range(cfg.num_seeds, dist.get_rank(), dist.get_world_size())
        if hi == lo:
            raise ValueError(f"{cfg.num_seeds} seeds cannot be sharded over {dist.get_world_size()} ranks")
        return cls(kin, scene, num_problems, dataclasses.replace(cfg, num_seeds=hi - lo), seed_offset=lo,
                   use_cuda_graph=use_cuda_graph, global_num_seeds=cfg.num_seeds)

    def _set_current_state(self, position: Optional[torch.Tensor], velocity: Optional[torch.Tensor], dt) -> None:
        """the current state of every problem into the fixed buffers of every rollout (row -> problem: the map the goals use);
        no position = dt 0: the terms are off"""
        if not self._with_state:
            return
        if position is None:
            position, velocity, dt = self._cur_buf, None, None
        for ro, rows in zip(self.rollouts + [self.metrics_rollout], self._row_goals + [self._mrow_goal]):
            ro.update_current_state(position, velocity, dt, rows)

    @property
    def _sp_on(self) -> bool:
        return float(self.cfg.rollout.support_polygon_weight) > 0.0

    def update_support_polygon(self, vertices_xy: torch.Tensor, padding: float = 0.05) -> None:
        """vertices_xy [1 | P, n, 2]: the points (e.g. the xy of the stance feet's spheres) whose padded convex hull the centre
        of mass is held over, one set for all problems or one per problem; written into the fixed buffers of every rollout
        (``IKRollout.update_support_polygon``), so the captured graphs stay valid unless the number of sets changes"""
        if not self._sp_on:
            raise ValueError("update_support_polygon: the solver was built with rollout.support_polygon_weight = 0")
        v = torch.as_tensor(vertices_xy).to(self.device, torch.float32)
        if v.dim() != 3 or int(v.shape[0]) not in (1, self.P):
            raise ValueError(f"update_support_polygon: vertices_xy must be (1 | {self.P}, n, 2), got {tuple(v.shape)}")
        n_sets = int(v.shape[0])
        if getattr(self, "_sp_sets", n_sets) != n_sets:
            self._drop_captures()  # (the rollouts allocate buffers for the new number of polygons)
        self._sp_sets = n_sets
        for ro, rows in zip(self.rollouts + [self.metrics_rollout], self._row_goals + [self._mrow_goal]):
            ro.update_support_polygon(v, None if n_sets == 1 else rows, padding)  # (rows: the global problem of every row)

    def reset_seed(self) -> None:
        """reference ``reset_seed``: rewind the Halton index stream of the LM seed stage, so that the next solve starts from
        the seeds the first solve started from"""
        if self.seed_solver is not None:
            self.seed_solver.reset_seed()

    def update_tool_pose_criteria(self, criteria) -> None:
        """``{tool frame: ToolPoseCriteria}`` for the L-BFGS stage and the success metrics (reference IKSolver.
        update_tool_pose_criteria); the LM seed stage keeps solving for the full pose -- its solutions are only seeds"""
        for ro in self.rollouts + [self.metrics_rollout]:
            ro.update_tool_pose_criteria(criteria)

    def sample_seeds(self) -> torch.Tensor:
        """[P, S, D] uniform in the joint limits; seed s of problem p depends only on its GLOBAL
        seed index so any sharding of the seed axis draws the same set."""
        lo, hi = self.kin.joint_limits_position[0].cpu(), self.kin.joint_limits_position[1].cpu()
        out = torch.empty(self.P, self.S, self.kin.num_dof)
        for s in range(self.S):
            self._gen.manual_seed(self.cfg.seed * 1000003 + self.seed_offset + s)
            out[:, s] = lo + (hi - lo) * torch.rand(self.P, self.kin.num_dof, generator=self._gen)
        return out.to(self.device)

    def solve_pose(self, goal_position: torch.Tensor, goal_quat: torch.Tensor,
                   seeds: Optional[torch.Tensor] = None, return_seeds: int = 1,
                   exit_early: Optional[bool] = None, env_idx: Optional[torch.Tensor] = None,
                   current_position: Optional[torch.Tensor] = None, current_velocity: Optional[torch.Tensor] = None,
                   dt=None) -> IKResult:
        """Goals of EVERY tool frame (reference IKSolver.solve_pose over a GoalToolPose, solver_ik.py:631-700): goal_position
        [P, T, G, 3], goal_quat [P, T, G, 4] (wxyz) with T = the robot's tool frames (``kin.tool_frames`` order) and G =
        ``cfg.num_goalset`` alternatives per problem (one member index per frame is chosen: the closest).  A robot with ONE
        tool frame also takes [P, 3] / [P, 4] or [P, G, 3] / [P, G, 4].  A solution succeeds when every frame is within the
        thresholds; the reported errors are the largest over the frames.  ``return_seeds`` k > 1 returns the k best seeds
        per problem, best first (solver_ik.py:503-530: top-k over the ranked cost), with a [P, k, ...] result.
        ``current_position`` [P, D]: the robot's configuration -- the first seed of every problem, and the seed stage prefers
        solutions close to it (reference: ``current_state`` / ``seed_config`` of solve_pose, as the MPC's goal IK passes them).
        With ``cfg.optimization_dt`` set it is also the state the solution has to be reachable from in ``dt`` (float or [P];
        default ``cfg.optimization_dt``), ``current_velocity`` [P, D] the velocity the acceleration regularisation refers to
        (None: at rest); without ``current_position`` the step is written as 0 and the solve is the plain one."""
        P, S, D, T, G = self.P, self.S, self.kin.num_dof, self.kin.num_pose_links, self.G
        if goal_position.numel() != P * T * G * 3 or goal_quat.numel() != P * T * G * 4:
            raise ValueError(f"solve_pose: expected goals for {P} problems x {T} tool frames {tuple(self.kin.tool_frames)} x {G} "
                             f"goal-set members, got position {tuple(goal_position.shape)}, quaternion {tuple(goal_quat.shape)}")
        gp = goal_position.to(self.device, torch.float32).reshape(P, T, G, 3).contiguous()
        gq = goal_quat.to(self.device, torch.float32).reshape(P, T, G, 4).contiguous()
        if dt is not None and not self._with_state:
            raise ValueError("solve_pose: dt needs a solver built with IKSolverCfg.optimization_dt")
        step = None
        if self._with_state and current_position is not None:
            step = self.cfg.optimization_dt if dt is None else dt
        self._set_envs(env_idx)
        self.metrics_rollout.update_goals(gp, gq, self._mrow_goal)
        self._set_current_state(current_position, current_velocity, step)
        if current_position is not None:
            self._cur_buf.copy_(current_position.to(self.device, torch.float32).reshape(P, D))
            self._cur_w.fill_(float(self.cfg.start_cspace_dist_weight))
            self._cur_on = True
        else:
            self._cur_on = False
        optimizer_goals_set = False

        def set_optimizer_goals():  # (only when the L-BFGS stage runs: with exit_early the seed solutions usually suffice)
            nonlocal optimizer_goals_set
            if not optimizer_goals_set:
                for ro, rows in zip(self.rollouts, self._row_goals):
                    ro.update_goals(gp, gq, rows)
                optimizer_goals_set = True
        if seeds is None:
            if self.seed_solver is not None:
                # the S_global best LM runs over all ranks, identical everywhere; this rank optimises its rows of them
                m = self.metrics_rollout  # (its goal buffers are the seed stage's: update_goals above filled them)
                shared = self.seed_solver.goal_position is m.goal_position
                cur = None if current_position is None else current_position.to(self.device, torch.float32).reshape(P, D)
                seeds = self.seed_solver.solve_batch(m.goal_position if shared else gp, m.goal_quat if shared else gq,
                                                     return_seeds=self.S_global, current_position=cur, dt=step,
                                                     current_velocity=current_velocity if step is not None else None).solution
                if self.S_global != S:
                    seeds = seeds[:, self.seed_offset:self.seed_offset + S].contiguous()
            else:
                seeds = self.sample_seeds()
        self.optimizer_ran = True
        if self.cfg.exit_early if exit_early is None else exit_early:
            early = self._get_result(seeds.reshape(P * S, D).contiguous(), return_seeds)
            solved = early.success if return_seeds == 1 else early.success[:, 0]
            if int(torch.count_nonzero(solved)) >= self.cfg.exit_early_batch_success_threshold * solved.numel():
                self.optimizer_ran = False
                return early
        set_optimizer_goals()
        best = self.optimizer.optimize(seeds.reshape(P * S, 1, D))
        return self._get_result(best.reshape(P * S, D).contiguous(), return_seeds)

    def _drop_captures(self) -> None:
        """every graph this solver replays is recorded again on next use"""
        self.optimizer.reset_cuda_graph()
        self._result_graphs.clear()

    def _set_envs(self, env_idx: Optional[torch.Tensor]) -> None:
        """``env_idx`` [P]: problem p is checked against scene environment env_idx[p] (reference batch-env
        IK, ``idxs_env`` / ``use_multi_env``); every rollout row takes the environment of its problem."""
        mode = env_idx is not None
        if not mode and getattr(self, "_env_mode", None) is False:
            return  # still "every row in environment 0": the index buffers are zero already (five fill launches per solve otherwise)
        env = env_idx.to(self.device).long().view(self.P) if mode else None
        rollouts = self.rollouts + [self.metrics_rollout]
        for ro, rows in zip(rollouts, self._row_goals + [self._mrow_goal]):
            ro.update_env_query_idx(env[rows.long()] if mode else None)
        # the mode and every rollout's choice of its fused launch (made in update_env_query_idx) decide the recorded launches
        launches = (mode, [ro._env_runs_ok for ro in rollouts])
        if launches != getattr(self, "_env_launches", (False, [True] * len(rollouts))):
            self._drop_captures()
        self._env_mode, self._env_launches = mode, launches

    def _get_result(self, q: torch.Tensor, return_seeds: int) -> IKResult:
        """``_get_result_eager`` replayed from a hipGraph when the process is alone (the ~25 small launches of the
        metrics + ranking are then one submission; with ``torch.distributed`` initialised the winner exchange is a
        collective and the eager path runs).  Results are copies: the next call does not overwrite them."""
        import torch.distributed as dist

        if not self._use_graph or (dist.is_available() and dist.is_initialized()):
            return self._get_result_eager(q, return_seeds)
        key = (return_seeds, bool(getattr(self, "_cur_on", False)))
        if key not in self._result_graphs:
            q_static = q.clone()
            graph, out = capture_graph(lambda: self._get_result_eager(q_static, return_seeds), device=self.device)
            self._result_graphs[key] = (graph, q_static, out, getattr(self, "_rank_pack", None))
        graph, q_static, out, pack = self._result_graphs[key]
        q_static.copy_(q)
        graph.replay()
        fields = ("success", "solution", "position_error", "rotation_error", "cost", "seed_index", "goalset_index")
        if pack is not None and getattr(out, "_packed", False):
            # the seven outputs of the ranking launch are views of ONE buffer: one copy instead of seven
            from .seed_ik import _unpack_like

            views = _unpack_like(out._pack_views, pack.clone())
            sq = (lambda x: x) if return_seeds > 1 else (lambda x: x[:, 0])  # noqa: E731
            spd = out.support_polygon_distance
            return IKResult(**{f: sq(v) for f, v in zip(fields, views)}, support_polygon_distance=None if spd is None else spd.clone())
        fields += ("support_polygon_distance",)
        return IKResult(**{f: (getattr(out, f).clone() if getattr(out, f) is not None else None) for f in fields})

    def _get_result_eager(self, q: torch.Tensor, return_seeds: int) -> IKResult:
        """Metrics of P*S joint configurations, feasibility checks and the ranked winner(s) per problem
        (reference IKSolver._get_result, solver_ik.py:440-580)."""
        P, S, D, T = self.P, self.S, self.kin.num_dof, self.kin.num_pose_links
        m = self.metrics_rollout
        cost = m.evaluate(q.view(P * S, 1, D), with_gradient=False)
        # with the robot's configuration given: ranked by pose errors + weight x 0.5 |q - current|^2 instead of the rollout's cost.
        # Ranks, does not decide success; the configuration lives in a fixed buffer the captured graph reads
        if getattr(self, "_cur_on", False):  # (the captured ranking graphs are keyed by this flag: no extra launches without it)
            near = (q.view(P, S, D) - self._cur_buf.view(P, 1, D)).square().sum(-1).reshape(P * S)
            cost = m.pose_pos_dist.view(P * S, T).sum(-1) + m.pose_rot_dist.view(P * S, T).sum(-1) + 0.5 * self._cur_w * near
        import torch.distributed as dist

        # the support-polygon term on: a seed whose centre of mass is outside its polygon (signed distance > 0) is infeasible,
        # next to the self, scene and c-space checks; folded into the self-collision row the ranking reads (both are >= 0)
        sp_dist = m.sp_distance.view(P, S) if self._sp_on else None
        self_dist = m.self_dist.view(P * S) if sp_dist is None else m.self_dist.view(P * S) + sp_dist.reshape(P * S).clamp_min(0.0)
        if not (dist.is_available() and dist.is_initialized()) and S <= 1024 and return_seeds <= S:
            # alone in the process: feasibility, success and the ranked winners in one launch (the winner exchange
            # below is only needed across ranks)
            from ..backends import linalg as linalg_hip

            from .seed_ik import _packed_outputs

            k, dev = return_seeds, self.device
            # (views of ONE buffer: a caller that wants copies -- _get_result over the replayed graph -- makes one)
            self._rank_pack, (ok_o, sol_o, pe_o, re_o, c_o, si_o, gi_o) = _packed_outputs(
                dev, [((P, k), torch.uint8), ((P, k, D), torch.float32), ((P, k), torch.float32), ((P, k), torch.float32),
                      ((P, k), torch.float32), ((P, k), torch.int64), ((P, k, T), torch.int64)])
            linalg_hip.ik_rank(ok_o, sol_o, pe_o, re_o, c_o, si_o, gi_o, q.view(P * S, D), cost.view(P * S), m.pose_pos_dist.view(P * S, T),
                               m.pose_rot_dist.view(P * S, T), self_dist, m.cspace_cost.view(P * S, D),
                               m.scene_dist if self.scene is not None else None, m.goalset_idx.view(P * S, T),
                               self.cfg.position_threshold, self.cfg.rotation_threshold, P, S, k, self.seed_offset)
            sq = (lambda x: x) if k > 1 else (lambda x: x[:, 0])  # noqa: E731
            ok_b = ok_o.view(torch.bool)  # (the kernel writes 0 / 1 bytes)
            res = IKResult(success=sq(ok_b), solution=sq(sol_o), position_error=sq(pe_o), rotation_error=sq(re_o),
                           cost=sq(c_o), seed_index=sq(si_o), goalset_index=sq(gi_o))
            res._packed, res._pack_views = True, [ok_b, sol_o, pe_o, re_o, c_o, si_o, gi_o]
            if sp_dist is not None:
                res.support_polygon_distance = sq(sp_dist.gather(1, (si_o - self.seed_offset).clamp(0, S - 1)))
            return res
        pos_all, rot_all = m.pose_pos_dist.view(P, S, T), m.pose_rot_dist.view(P, S, T)
        pos_err, rot_err = pos_all.max(-1).values, rot_all.max(-1).values  # the largest error over the tool frames
        feasible = (self_dist.view(P, S) <= 0.0) & (m.cspace_cost.view(P, S, D).sum(-1) <= 0.0)
        if self.scene is not None:
            feasible &= m.scene_dist.view(P, S, -1).sum(-1) <= 0.0
        # converged on every tool frame (reference: torch.all over the per-link convergence list, solver_ik.py:463-476)
        ok = feasible & (pos_all < self.cfg.position_threshold).all(-1) & (rot_all < self.cfg.rotation_threshold).all(-1)
        ranked = cost.view(P, S) + 1e16 * (~ok).float()  # reference solver_ik.py:503-509
        gidx = m.goalset_idx.view(P, S, T).float()
        payload = torch.cat([q.view(P, S, D), pos_err.unsqueeze(-1), rot_err.unsqueeze(-1), ok.float().unsqueeze(-1),
                             cost.view(P, S, 1), gidx] + ([sp_dist.unsqueeze(-1)] if sp_dist is not None else []), dim=-1)
        if return_seeds > 1:
            _, idx, win = global_topk(ranked, payload, self.seed_offset, return_seeds)
        else:
            _, idx, win = global_argmin(ranked, payload, self.seed_offset)
        return IKResult(success=win[..., D + 2] > 0.5, solution=win[..., :D], position_error=win[..., D],
                        rotation_error=win[..., D + 1], cost=win[..., D + 3], seed_index=idx,
                        goalset_index=win[..., D + 4:D + 4 + T].long(),
                        support_polygon_distance=win[..., D + 4 + T] if sp_dist is not None else None)
