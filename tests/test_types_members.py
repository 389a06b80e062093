"""Host types without the reference checkout: the members of ``JointState`` / ``ToolPose`` / ``GoalToolPose`` that the CPU harness holds to
the reference's classes (tests/golden/compare_joint_state.py, compare_goal_tool_pose.py) checked here against their definitions, so that
the suite covers them on a machine that has only this repository."""
import os

import pytest
import torch

from curobo_amd.kinematics import ToolPose
from curobo_amd.types import DeviceCfg, GoalToolPose, JointState


def _js(*shape, dt=None, names=True):
    g = torch.Generator().manual_seed(sum(shape))
    r = lambda: torch.randn(*shape, generator=g)  # noqa: E731
    return JointState(r(), r(), r(), r(), [f"j{i}" for i in range(shape[-1])] if names else None, None if dt is None else torch.as_tensor(dt))


def test_joint_state_constructors_and_state_tensor():
    p = torch.randn(5, 6)
    js = JointState.from_position(p, [f"j{i}" for i in range(6)])
    assert torch.equal(js.position, p) and all(float(t.abs().max()) == 0 for t in (js.velocity, js.acceleration, js.jerk))
    z = JointState.zeros((3, 6), DeviceCfg(device=torch.device("cpu")))
    assert z.dt.shape == (3,) and float(z.dt.min()) == 1.0
    st = torch.randn(4, 9, 24)
    back = JointState.from_state_tensor(st, dof=6).get_state_tensor()
    assert torch.equal(back, st)
    a = _js(4, 9, 6)
    assert a.stack(a).shape == (4, 18, 6) and a.cat(a, 0).shape == (8, 9, 6)
    assert a.cat(a, -1).joint_names == a.joint_names * 2
    assert (a.device, a.dtype, a.ndim, len(a)) == (a.position.device, torch.float32, 3, 4)


def test_joint_state_indexing_follows_a_per_row_dt():
    a = _js(4, 9, 6, dt=[0.1, 0.2, 0.3, 0.4])
    assert a[2].position.shape == (9, 6) and a[2].dt.tolist() == pytest.approx([0.3])
    assert a[torch.tensor([0, 3])].dt.tolist() == pytest.approx([0.1, 0.4])
    assert a[1:3].dt.tolist() == pytest.approx([0.2, 0.3]) and a[[1, 2]].position.shape == (2, 9, 6)
    b = a.clone()
    b[torch.tensor([0, 2])] = a[torch.tensor([1, 3])]
    assert torch.equal(b.position[0], a.position[1]) and b.dt.tolist() == pytest.approx([0.2, 0.2, 0.4, 0.4])


def test_joint_state_time_scaling_and_finite_differences():
    a = _js(9, 6, dt=[0.1])
    s = a.scale_by_dt(a.dt, torch.tensor([0.2]))
    assert torch.allclose(s.velocity, a.velocity * 0.5) and torch.allclose(s.acceleration, a.acceleration * 0.25)
    assert torch.allclose(s.jerk, a.jerk * 0.125) and s.dt.tolist() == pytest.approx([0.2])
    assert torch.allclose(a.scale(0.5).jerk, a.jerk * 0.125)
    t = torch.linspace(0, 1, 11).view(1, 11, 1)
    q = JointState.from_position(t ** 2 * torch.ones(1, 1, 3))
    q.calculate_fd_from_position(torch.tensor([0.1]))
    assert q.velocity.shape == (1, 10, 3) and q.acceleration.shape == (1, 9, 3) and q.jerk.shape == (1, 8, 3)
    assert torch.allclose(q.acceleration, torch.full_like(q.acceleration, 2.0), atol=1e-3)  # d2/dt2 of t^2


def test_joint_state_reorder_append_and_augment():
    a = _js(4, 6)
    order = ["j3", "j0", "j5", "j1", "j2", "j4"]
    r = a.reorder(order)
    assert r.joint_names == order and torch.equal(r.position[:, 0], a.position[:, 3]) and a.joint_names[0] == "j0"
    assert a.reorder(order[:2]).position.shape == (4, 2)
    lock = JointState.from_position(torch.tensor([0.01, 0.02]), ["gl", "gr"])
    full = a.get_augmented_joint_state(["gr"] + order + ["gl"], lock)
    assert full.position.shape == (4, 8) and torch.all(full.position[:, 0] == 0.02) and torch.all(full.position[:, -1] == 0.01)
    assert float(full.velocity[:, 0].abs().max()) == 0.0
    assert _js(3, 5, 6).append_joints(lock).position.shape == (3, 5, 8) and _js(6).append_joints(lock).position.shape == (8,)
    with pytest.raises(ValueError):
        a.get_augmented_joint_state(order, JointState.from_position(torch.zeros(1), ["j0"]))
    with pytest.raises(ValueError):
        a.reorder(["j0", "nope"])
    assert a.index_dof(torch.tensor([4, 1])).joint_names == ["j4", "j1"]


def test_joint_state_seed_gather_trims_and_copies():
    a = _js(3, 5, 7, 6, dt=torch.rand(3, 5) + 0.01)
    idx = torch.tensor([[4, 0], [1, 1], [2, 3]])
    g = a.gather_by_seed_index(idx)
    assert g.position.shape == (3, 2, 7, 6) and torch.equal(g.position[1, 0], a.position[1, 1]) and torch.equal(g.dt[2], a.dt[2, [2, 3]])
    b = _js(4, 9, 6)
    assert torch.equal(b.get_trajectory_at_horizon_index(-1).position, b.position[:, -1])
    assert b.trim_trajectory(2, 7).position.shape == (4, 5, 6) and b.trim_trajectory(3).position.shape == (4, 6, 6)
    src = _js(4, 9, 6)
    c = b.clone()
    ptr = c.position.data_ptr()
    c.copy_(src)
    assert c.position.data_ptr() == ptr and torch.equal(c.position, src.position)  # in place when the shapes agree
    d = b.clone().copy_(_js(2, 6))
    assert d.position.shape == (2, 6)
    with pytest.raises(ValueError):
        b.clone().copy_(_js(2, 6), allow_clone=False)
    rs = _js(5, 6).repeat_seeds(3)
    assert rs.position.shape == (15, 6) and torch.equal(rs.position[0], rs.position[2]) and not torch.equal(rs.position[0], rs.position[3])


@pytest.mark.parametrize("cls,shape", [(ToolPose, (4, 3, 3)), (GoalToolPose, (4, 3, 3, 2))])
def test_frame_pose_members(cls, shape):
    frames = ["a", "b", "c"]
    p, q = torch.randn(*shape, 3), torch.randn(*shape, 4)
    x = cls(list(frames), p.clone(), q.clone())
    n = 1
    for s in shape[:2] + shape[3:]:
        n *= s
    assert x["b"].position.shape == (n, 3) and x.get_link_pose("c").name == "c" and list(x.to_dict()) == frames
    assert x[2].position.shape == (1, *shape[1:], 3) and x[torch.tensor([0, 3])].position.shape == (2, *shape[1:], 3)
    r = x.reorder_links(["c", "a"])
    assert r.tool_frames == ["c", "a"] and torch.equal(r.position[:, :, 0], p[:, :, 2]) and x.reorder_links(frames) is x
    assert len(x) == 3 and x.ndim == len(shape) + 1 and (x.batch_size, x.horizon, x.num_links) == (4, 3, 3)
    c = x.clone()
    c.position.zero_()
    assert float(x.position.abs().max()) > 0 and x.detach().position.data_ptr() == x.position.data_ptr()
    y = cls(list(frames), torch.zeros_like(p), torch.zeros_like(q))
    y.copy_(x)
    assert torch.equal(y.position, p) and torch.equal(y.quaternion, q)
    with pytest.raises(ValueError):
        x.get_link_pose("zz")
    with pytest.raises(ValueError):
        x.reorder_links(["a", "zz"])
    if cls is ToolPose:
        g = x.as_goal(["b", "a"])
        assert isinstance(g, GoalToolPose) and g.position.shape == (4, 3, 2, 1, 3) and g.tool_frames == ["b", "a"]


def test_seed_knot_placement_options():
    """``TrajOptSolver.seed_knots``: the default spacing and the reference's (util/trajectory_seed_generator.py:16-40: weights
    linspace(0, 1, n_knots), first free knot on the start, last on the goal), on a stand-in for the solver (pure torch, no device work)"""
    import types

    from curobo_amd.solver.trajopt import TrajOptSolver, TrajOptSolverCfg

    D, P, S, nk = 3, 2, 2, 5
    lim = torch.stack([torch.full((D,), -3.0), torch.full((D,), 3.0)])
    start, goal = torch.tensor([[0.0, 0.5, -0.5]]), torch.tensor([[[1.0, 1.5, 0.5]], [[-1.0, 0.0, 0.25]]])
    for placement, want_t in (("even", torch.linspace(0, 1, nk + 2)[1:-1]), ("reference", torch.linspace(0, 1, nk))):
        cfg = TrajOptSolverCfg(num_seeds=S, seed_knot_placement=placement, seed_bump=0.0)
        cfg.rollout.n_knots = nk
        stub = types.SimpleNamespace(cfg=cfg, kin=types.SimpleNamespace(num_dof=D, joint_limits_position=lim), P=P, S=S, S_global=S, device=torch.device("cpu"))
        k = TrajOptSolver.seed_knots(stub, start, goal)
        assert k.shape == (P, S, nk, D)
        want = start.view(1, 1, 1, D) * (1 - want_t.view(1, 1, nk, 1)) + goal.view(P, 1, 1, D) * want_t.view(1, 1, nk, 1)
        assert torch.allclose(k, want.expand(P, S, nk, D), atol=1e-6), placement
    # the reference's generator itself, when its checkout is here
    import os
    import sys

    if os.path.isdir("/root/reference/curobo"):
        code = ("import sys; sys.path.insert(0, '/root/reference'); import torch; "
                "from curobo._src.util.trajectory_seed_generator import interpolate_kernel; from curobo._src.types.device_cfg import DeviceCfg; "
                "w = interpolate_kernel(2, 5, DeviceCfg(device=torch.device('cpu'))); print(w[:, 1].tolist())")
        import subprocess

        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        if out.returncode == 0:  # (an import the stand-ins do not cover leaves the definition-based check above)
            assert eval(out.stdout.strip().splitlines()[-1]) == pytest.approx(torch.linspace(0, 1, nk).tolist())
    with pytest.raises(ValueError):
        cfg = TrajOptSolverCfg(num_seeds=S, seed_knot_placement="nope")
        cfg.rollout.n_knots = nk
        TrajOptSolver.seed_knots(types.SimpleNamespace(cfg=cfg, kin=types.SimpleNamespace(num_dof=D, joint_limits_position=lim), P=P, S=S, S_global=S,
                                                       device=torch.device("cpu")), start, goal)


def test_deceleration_knots_bring_the_robot_to_rest():
    """``util/deceleration.py`` by its definition (the reference's generator is compared in tests/golden/compare_deceleration_seeds.py) and
    ``MPCSolver.prepare_safe_deceleration_trajectory`` over a stand-in for the solver"""
    import types

    from curobo_amd.solver.mpc import MPCSolver, MPCSolverCfg
    from curobo_amd.util.deceleration import deceleration_accelerations, deceleration_knots

    p = torch.tensor([[0.0, 1.0, -1.0]])
    v = torch.tensor([[1.0, -0.5, 0.0]])
    a = torch.tensor([[2.0, 0.0, 3.0]])
    for profile in ("linear", "exponential", "smooth"):
        acc = deceleration_accelerations(v, a, 12, profile)
        assert torch.equal(acc[0, 0], torch.tensor([2.0, 0.0, 0.0]))  # starts from the current acceleration; a resting joint gets none
        assert bool((acc[0, 4:, 0] <= 0).all()) and bool((acc[0, 4:, 1] >= 0).all())  # then opposes the velocity
        k = deceleration_knots(p, v, a, 0.05, 12, profile)
        assert k.shape == (1, 12, 3) and torch.equal(k[:, 0], p) and torch.equal(k[0, :, 2], torch.full((12,), -1.0))
        step = k[0, 1:] - k[0, :-1]
        assert bool((step[:, 0] >= 0).all()) and bool((step[:, 1] <= 0).all())  # never reverses
        assert float(step[-1].abs().max()) <= float(step[0].abs().max())  # slower at the end than at the start
    cfg = MPCSolverCfg()
    stub = types.SimpleNamespace(cfg=cfg, rollout_cfg=types.SimpleNamespace(n_knots=12), kin=types.SimpleNamespace(num_dof=3), B=1, device=torch.device("cpu"))
    js = JointState(position=p, velocity=v, acceleration=a)
    k = MPCSolver.prepare_safe_deceleration_trajectory(stub, js, torch.tensor([True]))
    assert torch.equal(k, deceleration_knots(p, v, a, cfg.optimization_dt, 12, "exponential"))
    still = MPCSolver.prepare_safe_deceleration_trajectory(stub, JointState(position=p, velocity=v * 0, acceleration=a), torch.tensor([True]))
    assert torch.equal(still, p.view(1, 1, 3).expand(1, 12, 3))
    cfg.use_deceleration_on_failure = False
    assert torch.equal(MPCSolver.prepare_safe_deceleration_trajectory(stub, js, torch.tensor([True])), still)


def test_ik_result_clone_and_merges():
    """``InverseKinematicsResult.clone / copy_successful_solutions / copy_at_batch_indices`` (reference solver_base_result.py:81-240)"""
    from curobo_amd.solver.inverse_kinematics import InverseKinematicsResult

    def result(seed, success):
        g = torch.Generator().manual_seed(seed)
        sol = torch.randn(3, 2, 7, generator=g)
        return InverseKinematicsResult(success=torch.tensor(success), solution=sol, js_solution=JointState.from_position(sol.clone()),
                                       position_error=torch.rand(3, 2, generator=g), rotation_error=torch.rand(3, 2, generator=g),
                                       goalset_index=torch.zeros(3, 2, 1, dtype=torch.long), debug_info={"t": torch.ones(1), "n": 3}, batch_size=3, num_seeds=2)

    a = result(1, [[True, False], [False, False], [False, True]])
    b = result(2, [[False, True], [True, False], [False, True]])
    c = a.clone()
    c.solution.zero_(), c.debug_info["t"].zero_()
    assert float(a.solution.abs().max()) > 0 and float(a.debug_info["t"]) == 1.0 and c.batch_size == 3
    m = a.clone()
    m.copy_successful_solutions(b)
    assert m.success.tolist() == [[True, True], [True, False], [False, True]]
    assert torch.equal(m.solution[0, 1], b.solution[0, 1]) and torch.equal(m.solution[0, 0], a.solution[0, 0])
    assert torch.equal(m.solution[2, 1], b.solution[2, 1]) and torch.equal(m.js_solution.position[1, 0], b.solution[1, 0])
    assert float(m.position_error[1, 0]) == float(b.position_error[1, 0]) and float(m.position_error[1, 1]) == float(a.position_error[1, 1])
    w = a.clone()
    w.copy_at_batch_indices(b, torch.tensor([False, True, False]))
    assert torch.equal(w.solution[1], b.solution[1]) and torch.equal(w.solution[0], a.solution[0]) and w.success[1].tolist() == [True, False]
    assert torch.equal(w.js_solution.position[1], b.solution[1])


REF_CUROBO = "/root/reference/curobo"
REF_TASKS = os.path.join(REF_CUROBO, "content", "configs", "task")
# the values these tests read from the reference's task files (and its MPCSolverCfg iteration counts), recorded from them
REF_TASK_VALUES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_task_configs.json")


def _reference_task_file(name):
    """the recorded blocks of a reference task file (``name`` relative to content/configs/task) or ``solver_mpc_cfg``; where
    the reference checkout is present, the record must still match the files themselves"""
    import json
    import re

    import yaml

    with open(REF_TASK_VALUES) as fh:
        rec = json.load(fh)[name]
    if os.path.isdir(REF_TASKS):
        if name == "solver_mpc_cfg":
            src = open(os.path.join(REF_CUROBO, "_src", "solver", "solver_mpc_cfg.py")).read()
            live = {k: int(re.search(rf"{k}: int = (\d+)", src).group(1)) for k in rec}
        else:
            with open(os.path.join(REF_TASKS, name)) as fh:
                y = yaml.safe_load(fh)
            live = {k: ({kk: y[k][kk] for kk in rec[k]} if k == "rollout" else y[k]) for k in rec}
            live = {k: ({kk: {n: v[kk][n] for n in rec[k][kk]} for kk in v} if k == "rollout" else v) for k, v in live.items()}
        assert json.loads(json.dumps(live)) == rec, f"{REF_TASK_VALUES} is stale for {name}"
    return rec


def test_mpc_reference_task_is_the_reference_file():
    """``MPCSolverCfg.reference_task()`` against content/configs/task/mpc/lbfgs_mpc.yml, value by value (this package's own MPC defaults differ
    from that file on purpose; the option carries the file's)"""
    import os

    import yaml

    from curobo_amd.solver.mpc import MPCSolverCfg

    c = MPCSolverCfg.reference_task(goal_ik_seeds=8)
    assert c.goal_ik_seeds == 8 and c.rollout.non_terminal_pose_factor == 1.0
    y = _reference_task_file("mpc/lbfgs_mpc.yml")
    cost, con, opt = y["rollout"]["cost_cfg"], y["rollout"]["constraint_cfg"], y["optimizer"]
    r, o = c.rollout, c.optimizer
    cs = cost["cspace_cfg"]
    assert [float(v) for v in cs["weight"]] == r.cspace_weight and [float(v) for v in cs["activation_distance"]] == r.cspace_activation_distance
    assert [float(v) for v in cs["squared_l2_regularization_weight"]] == r.cspace_regularization
    assert (cs["retime_weights"], cs["retime_regularization_weights"]) == (r.retime_weights, r.retime_regularization_weights)
    assert (float(cs["cspace_target_weight"]), float(cs["cspace_non_terminal_weight_factor"])) == (r.cspace_target_weight, r.cspace_non_terminal_weight_factor)
    tp = cost["tool_pose_cfg"]
    assert [float(v) for v in tp["weight"]] == r.pose_weight and [float(v) for v in tp["_terminal_pose_convergence_tolerance"]] == r.pose_convergence_tolerance
    assert tp["use_lie_group"] is False and r.rotation_method == 0
    sc = con["scene_collision_cfg"]
    assert (float(sc["activation_distance"]), float(sc["weight"]), sc["use_sweep"], sc["use_speed_metric"]) == \
        (r.scene_activation_distance, r.scene_collision_weight, r.use_sweep, r.use_speed_metric)
    assert float(con["self_collision_cfg"]["weight"]) == r.self_collision_weight
    assert (opt["history"], opt["inner_iters"], opt["num_iters"]) == (o.history, o.inner_iters, o.num_iters)
    assert [float(v) for v in opt["line_search_scale"]] == o.line_search_scale and opt["line_search_type"] == o.line_search_type
    assert (float(opt["line_search_wolfe_c_1"]), float(opt["line_search_wolfe_c_2"])) == (o.line_search_c_1, o.line_search_c_2)
    assert (float(opt["cost_relative_threshold"]), float(opt["epsilon"]), float(opt["step_scale"]), opt["stable_mode"], opt["fixed_iters"]) == \
        (o.cost_relative_threshold, o.epsilon, o.step_scale, o.stable_mode, o.fixed_iters)
    # ... which reaches the kernels as the reference's optimiser hands it over: with fixed_iters both improvement thresholds are zero
    # (optim/gradient/gradient_descent.py:68-75); the file's 1.0 taken literally freezes the best iterate at the seed
    assert o.improvement_thresholds() == (0.0, 0.0)
    import dataclasses
    with pytest.raises(ValueError):
        dataclasses.replace(o, fixed_iters=False).improvement_thresholds()
    assert dataclasses.replace(o, fixed_iters=False, cost_relative_threshold=0.01).improvement_thresholds() == (0.0, 0.01)
    # the iteration counts are those of the reference's MPCSolverCfg (solver_mpc_cfg.py:75-78)
    it = _reference_task_file("solver_mpc_cfg")
    warm, cold = it["warm_start_optimization_num_iters"], it["cold_start_optimization_num_iters"]
    assert (c.cold_start_optimization_num_iters, c.warm_start_optimization_num_iters) == (cold, warm) == (300, 200)


@pytest.mark.parametrize("task,path", [("ik", "ik/particle_ik.yml"), ("trajopt", "trajopt/particle_trajopt.yml")])
def test_mppi_reference_tasks_are_the_reference_files(task, path):
    """``MPPICfg.reference_task`` against the optimiser block of the reference's particle-stage task files, value by value"""
    import os

    import yaml

    from curobo_amd.optim.mppi import MPPICfg

    c = MPPICfg.reference_task(task, num_problems=3)
    assert c.num_problems == 3
    with pytest.raises(ValueError):
        MPPICfg.reference_task("mpc")
    o = _reference_task_file(path)["optimizer"]
    for k in ("gamma", "init_cov", "kappa", "beta", "step_size_cov", "step_size_mean", "null_act_frac"):
        assert float(o[k]) == getattr(c, k), k
    for k in ("num_iters", "inner_iters", "num_particles", "sample_per_problem", "seed", "update_cov"):
        assert o[k] == getattr(c, k), k
    assert o["sample_mode"] == c.sample_mode and o["solver_type"] == "mppi"
    sp = o["sample_params"]
    assert tuple(float(v) for v in sp["filter_coeffs"]) == c.filter_coeffs and sp["fixed_samples"] == c.fixed_samples
    assert {k: float(v) for k, v in sp["sample_ratio"].items() if float(v) > 0} == c.sample_ratio


def test_solvers_say_once_what_the_reference_mesh_gradient_does():
    """a solver over a hand-built mesh store in the reference's gradient mode warns (once per process); a store in the consistent
    mode -- what ``scene_from_config`` builds -- does not"""
    import warnings

    from curobo_amd.scene import data as D

    class Store:
        def __init__(self, mode):
            self.gradient_mode = mode

    class Scene:
        def __init__(self, mode):
            self.meshes = Store(mode)

    D.warn_if_reference_mesh_gradient._said = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        D.warn_if_reference_mesh_gradient(None, "TrajOptSolver")
        D.warn_if_reference_mesh_gradient(Scene(1), "TrajOptSolver")
        assert len(w) == 0
        D.warn_if_reference_mesh_gradient(Scene(0), "TrajOptSolver")
        D.warn_if_reference_mesh_gradient(Scene(0), "IKSolver")
        assert len(w) == 1 and "gradient_mode 0" in str(w[0].message) and "CONSISTENT_GRADIENT" in str(w[0].message)
