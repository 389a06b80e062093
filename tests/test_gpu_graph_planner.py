"""PRM graph planner on the GPU: the fused steering launch against the materialised reference path and against the float64 oracle
(oracle/graph_ref.py, batches of tests/graph_cases.py, conditions held on the CPU by tests/test_oracle_graph.py), the k-NN launch
against fp64 NumPy, a narrow-passage query and the MotionPlanner wiring."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THR = 0.005


def _checker(device, robot, world):
    from curobo_amd.collision_checking import RobotCollisionChecker
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c2_world, c3_voxel_world

    kin = KinematicsCfg.from_packaged(robot, device=device)
    if world == "c2":
        scene = SceneData.from_arrays(cuboid_scene_arrays(c2_world()), device)
    elif world == "c3":
        scene = SceneData.from_arrays(c3_voxel_world(), device)
    elif world == "primitives":
        from curobo_amd.scene.config import scene_from_config

        from graph_cases import PRIMITIVE_WORLD

        scene = scene_from_config(PRIMITIVE_WORLD, device)
        assert scene.struct.cuboid_has_primitives
    else:
        scene = None
    return RobotCollisionChecker(kin, scene, 0.0)


def _edges(checker, n, seed):
    from curobo_amd.solver.seed_ik import HaltonSeeds

    lim = checker.kinematics.kinematics_config.joint_limits_position
    lo, hi = lim[0].contiguous(), lim[1].contiguous()
    hs = HaltonSeeds(lo.numel(), lo, hi, seed=seed)
    s, t = hs.get_samples(n), hs.get_samples(n)
    t = s + 0.15 * (t - s)  # mostly short edges (roadmap-like), plus:
    t[:40] = s[:40]  # zero-length edges
    t[40:80] = s[40:80] + 0.3 * (hi - lo)  # edges that leave the joint limits
    s[80] = lo + 0.05 * (hi - lo)  # one long edge: sets the batch-wide step count
    t[80] = hi - 0.05 * (hi - lo)
    return s.contiguous(), t.contiguous()


@pytest.mark.parametrize("robot,world", [("franka", "c2"), ("franka", "primitives"), ("ur10e", "c3"), ("dual_ur10e", None)])
def test_steering_matches_the_materialised_path(device, robot, world):
    from curobo_amd.graph_planner.prm import GraphFeasibility, last_feasible_index, steer_num_steps, steer_points

    checker = _checker(device, robot, world)
    D = checker.kinematics.kinematics_config.num_dof
    w = torch.ones(D, device=device)
    s, t = _edges(checker, 2000, seed=11)
    feas = GraphFeasibility(checker, THR, w, 2000)
    assert feas.uses_fused()
    node, idx = feas.steer(s, t)
    torch.cuda.synchronize()
    ms = int(steer_num_steps(s, t, w, THR).max().item())
    pts = steer_points(s, t, ms)
    mask = torch.cat([checker.validate(c.unsqueeze(1)).view(-1) for c in pts.reshape(-1, D).split(65536)]).view(-1, ms + 1)
    ref = last_feasible_index(mask)
    start_bad = int((~mask[:, 0]).sum())
    some_bad = int((~mask.all(1)).sum())
    assert start_bad > 0 and some_bad > start_bad and int(mask.all(1).sum()) > 0, (start_bad, some_bad)  # every case present
    diff = (idx.long() != ref)
    assert int(diff.sum()) == 0, f"{int(diff.sum())} of {len(ref)} edges disagree: {torch.nonzero(diff)[:10].view(-1).tolist()}"
    want = pts[torch.arange(len(ref), device=device), ref]
    torch.testing.assert_close(node[:, :D], want, atol=1e-6, rtol=0)
    assert bool((node[:, D] == 0).all())
    # point mode: the start of every edge
    torch.testing.assert_close(feas.feasible(s), mask[:, 0])


@pytest.mark.parametrize("D", [7, 12])
def test_knn_matches_fp64_numpy(device, D):
    from curobo_amd.backends import graph as graph_hip

    g = np.random.default_rng(D)
    N, Q = 20000, 256
    nodes = g.uniform(-2, 2, (N, D + 1)).astype(np.float32)
    nodes[N // 2:N // 2 + 500, :D] = nodes[100:600, :D]  # duplicated nodes: exact ties
    queries = np.concatenate([g.uniform(-2, 2, (Q - 16, D)), nodes[100:116, :D]]).astype(np.float32)
    w = g.uniform(0.5, 1.5, D).astype(np.float32)
    dist = (((nodes[None, :, :D].astype(np.float64) - queries[:, None].astype(np.float64)) * w.astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(dist, axis=1, kind="stable")
    tn, tq, tw = (torch.as_tensor(x, device=device) for x in (nodes, queries, w))
    for k in (1, 10, 32):
        out = torch.empty(Q, k, dtype=torch.int32, device=device)
        graph_hip.graph_knn(out, tq, tn, tw, N, D, k)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got, order[:, :k])
    # only the first n_nodes are searched
    out = torch.empty(Q, 4, dtype=torch.int32, device=device)
    graph_hip.graph_knn(out, tq, tn, tw, 1000, D, 4)
    np.testing.assert_array_equal(out.cpu().numpy(), np.argsort(dist[:, :1000], axis=1, kind="stable")[:, :4])


# ---------------------------------------------------------------------------------------------- against the float64 oracle
_CHECKERS = {}


def _oracle_checker(device, robot, scene):
    import graph_cases as gc

    if (robot, scene) not in _CHECKERS:
        _CHECKERS[(robot, scene)] = gc.build_checker(device, robot, scene)
    return _CHECKERS[(robot, scene)]


def _oracle_pairs():
    import graph_cases as gc

    return gc.oracle_pairs()


@pytest.mark.parametrize("robot,scene", _oracle_pairs(), ids=lambda v: str(v))
def test_steering_matches_the_oracle(device, robot, scene):
    """max_steps exact; out_index equal to the oracle's on every edge its band decides and inside the band's span on the others
    (at most 5 % of the batch, asserted again here); out_node the fp32 point formula at the returned index.  The cases lie on both
    sides of the launch's 60 KiB LDS branch: dual_ur10e with the 64-slot scene needs 62 400 bytes, every other pair less
    (tests/test_oracle_graph.py::test_cases_lie_on_both_sides_of_the_60_kib_launch_path; of the packaged robots none comes nearer,
    unitree_g1 does not fit the fused launch at all and is left out by ``GraphFeasibility.uses_fused``)."""
    import graph_cases as gc
    from curobo_amd.graph_planner.prm import GraphFeasibility

    checker = _oracle_checker(device, robot, scene)
    case = gc.oracle_case(robot, scene)
    assert GraphFeasibility(checker, case["threshold"], torch.as_tensor(case["weight"], device=device), 2000).uses_fused()
    lds = [gc.fused_lds_bytes(*p) for p in gc.oracle_pairs()]
    assert min(lds) < 60 * 1024 < max(lds)
    ref = gc.steering_reference(case)
    node, idx, ms = gc.run_steer(checker, case)
    share = gc.check_steer(ref, node, idx, ms)
    print(f"{robot} / {scene}: max_steps {ms}, undecided {100 * share:.2f} %, LDS {gc.fused_lds_bytes(robot, scene)} bytes")
    # the planner's entry point gives the same answer
    feas = GraphFeasibility(checker, case["threshold"], torch.as_tensor(case["weight"], device=device), 2000)
    node2, idx2 = feas.steer(torch.as_tensor(case["start"], device=device), torch.as_tensor(case["target"], device=device))
    np.testing.assert_array_equal(idx2.cpu().numpy(), idx)
    np.testing.assert_array_equal(node2.cpu().numpy().view(np.int32), node.view(np.int32))


@pytest.mark.parametrize("n_pts", [16, 17, 40])
def test_steering_placed_crossings(device, n_pts):
    """one joint crosses a limit with the first violating step k* placed at 0, 1, 15, 16, 17, 31, 32 and max_steps (those that the
    point count admits): index max(k* - 1, 0), as literals"""
    import graph_cases as gc

    literal = {16: [15] + 8 * [0] + 4 * [14], 17: [16] + 8 * [0] + 4 * [14] + 4 * [15],
               40: [39] + 8 * [0] + 4 * [14] + 4 * [15] + 4 * [16] + 4 * [30] + 4 * [31] + 4 * [38]}[n_pts]
    case = gc.placed_crossings(n_pts)
    ref = gc.steering_reference(case)
    assert ref["band"]["decided"].all() and ref["band"]["index"].tolist() == literal
    node, idx, ms = gc.run_steer(_oracle_checker(device, "franka", "none"), case)
    assert ms == n_pts - 1
    assert idx.tolist() == literal, (case["kstar"].tolist(), idx.tolist())
    gc.check_steer(ref, node, idx, ms)


def test_steering_zero_length_batch(device):
    import graph_cases as gc
    from oracle.graph_ref import FEASIBLE

    case = gc.zero_length_batch()
    ref = gc.steering_reference(case)
    node, idx, ms = gc.run_steer(_oracle_checker(device, "franka", "c2"), case)
    assert ms == 1
    gc.check_steer(ref, node, idx, ms)
    dec = ref["band"]["decided"]
    np.testing.assert_array_equal(idx[dec], np.where(ref["band"]["state"][dec, 0] == FEASIBLE, 1, 0))
    assert set(idx.tolist()) == {0, 1}
    np.testing.assert_array_equal(node[:, :7], case["start"])  # (t == s: every point is the start, bit for bit)


def test_steering_beyond_the_grid(device):
    """2048 + 37 edges: the first 37 workgroups walk a second edge, carrying ``first_bad`` and the barrier handshake over"""
    import graph_cases as gc

    case = gc.beyond_the_grid()
    ref = gc.steering_reference(case)
    node, idx, ms = gc.run_steer(_oracle_checker(device, "franka", "c2"), case)
    gc.check_steer(ref, node, idx, ms)
    dec, want = ref["band"]["decided"], ref["band"]["index"]
    for part in (slice(0, gc.GRID_CAP), slice(gc.GRID_CAP, None)):
        assert (want[part][dec[part]] == 0).any() and (want[part][dec[part]] == ms).any() and ((want[part][dec[part]] > 0) & (want[part][dec[part]] < ms)).any()


@pytest.mark.parametrize("pad", [1, 3])
def test_steering_row_stride(device, pad):
    """rows of ld = D + 1 and D + 3 floats with NaN in the padding: bit-identical to contiguous rows, edge and point mode"""
    import graph_cases as gc

    case = gc.row_stride_case()
    checker = _oracle_checker(device, "franka", "c2")
    node, idx, ms = gc.run_steer(checker, case)
    gc.check_steer(gc.steering_reference(case), node, idx, ms)
    D = case["weight"].shape[0]
    node_p, idx_p, ms_p = gc.run_steer(checker, case, ld=D + pad)
    assert ms_p == ms
    np.testing.assert_array_equal(idx_p, idx)
    np.testing.assert_array_equal(node_p.view(np.int32), node.view(np.int32))
    np.testing.assert_array_equal(gc.run_points(checker, case["start"], ld=D + pad), gc.run_points(checker, case["start"]))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 32768 + 5])
def test_point_feasibility_matches_the_oracle(device, n):
    """16 configurations per workgroup: partly filled workgroups, and 32768 + 5 points for a second pass of the 2048 workgroups"""
    import graph_cases as gc
    from curobo_amd.graph_planner.prm import GraphFeasibility

    assert n in gc.POINT_SIZES
    c = gc.point_batch(n)
    checker = _oracle_checker(device, c["robot"], c["scene"])
    flags = gc.run_points(checker, c["q"])
    share = gc.check_points(gc.points_reference(n), flags)
    print(f"points {n}: undecided {100 * share:.3f} %")
    feas = GraphFeasibility(checker, gc.THRESHOLD, torch.ones(7, device=device), 2000)
    np.testing.assert_array_equal(feas.feasible(torch.as_tensor(c["q"], device=device)).cpu().numpy(), flags.astype(bool))


def _knn_ids():
    import graph_cases as gc

    return gc.knn_ids()


@pytest.mark.parametrize("name", _knn_ids())
def test_knn_edges(device, name):
    """1 / 63 / 64 / 65 nodes, k = 64 and k == n_nodes, 1 / 5 / 255 queries, 1 / 7 / 12 joints, queries as rows of the node buffer
    (ld_q = D + 1) past the searched prefix, exact grid values with plentiful ties: equal to the stable float64 reference"""
    import graph_cases as gc

    c = gc.knn_set(name)
    got = gc.run_knn(device, c)
    gc.check_knn(c, got)
    if name == "identical":
        np.testing.assert_array_equal(got, np.tile(np.arange(64, dtype=np.int32), (got.shape[0], 1)))


WALL = {"table": {"dims": [2.0, 2.0, 0.2], "pose": [0.0, 0.0, -0.1, 1, 0, 0, 0]},
        "pillar": {"dims": [0.16, 0.16, 0.7], "pose": [0.5, 0.0, 0.35, 1, 0, 0, 0]}}
Q0 = [-0.9, 0.3, 0.0, -1.9, 0.0, 2.2, 0.8]


def _wall_problem(device):
    q0 = torch.tensor([Q0], device=device)
    q1 = q0.clone()
    q1[0, 0] = 0.9  # the straight joint-space line sweeps the outstretched arm through the pillar
    return q0, q1


def _check_paths(planner, checker, r):
    from curobo_amd.graph_planner.prm import steer_num_steps, steer_points

    D = planner.action_dim
    for p in r.plan_waypoints:
        for a, b in zip(p[:-1], p[1:]):
            ms = max(int(steer_num_steps(a.view(1, D), b.view(1, D), planner.cspace_distance_weight, THR).item()), 1)
            pts = steer_points(a.view(1, D), b.view(1, D), ms).view(-1, D)
            assert bool(checker.validate(pts.unsqueeze(1)).all())


def test_narrow_passage_find_path(device):
    from curobo_amd.collision_checking import RobotCollisionChecker
    from curobo_amd.graph_planner import PRMGraphPlanner, PRMGraphPlannerCfg
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.scene.config import scene_from_config

    kin = KinematicsCfg.from_packaged("franka", device=device)
    checker = RobotCollisionChecker(kin, scene_from_config({"cuboid": WALL}, device), 0.0)
    q0, q1 = _wall_problem(device)
    tt = torch.linspace(0, 1, 200, device=device).view(-1, 1)
    assert not bool(checker.validate((q0 * (1 - tt) + q1 * tt).unsqueeze(1)).all()), "the straight line must be infeasible"
    planner = PRMGraphPlanner(PRMGraphPlannerCfg(), checker)
    r = planner.find_path(q0, q1, interpolation_steps=32)
    assert bool(r.success.all()), r.debug_info
    assert r.interpolated_waypoints.shape == (1, 32, 7)
    _check_paths(planner, checker, r)
    assert planner.n_nodes > 2 and planner.graph.num_edges > 0
    first = r.plan_waypoints[0].clone()
    planner.reset_buffer()
    planner.reset_seed()
    r2 = planner.find_path(q0, q1, interpolation_steps=32)
    assert bool(r2.success.all()) and torch.equal(r2.plan_waypoints[0], first)
    # the mesh fallback (materialised steering through checker.validate) on the same wall built as a mesh
    from curobo_amd.scene.primitives import box_mesh

    vb, fb = box_mesh([0.16, 0.16, 0.7])
    mscene = scene_from_config({"cuboid": {"table": WALL["table"]},
                                "mesh": {"pillar": {"vertices": vb, "faces": fb, "pose": WALL["pillar"]["pose"]}}}, device)
    mchecker = RobotCollisionChecker(kin, mscene, 0.0)
    mplanner = PRMGraphPlanner(PRMGraphPlannerCfg(), mchecker)
    assert not mplanner.feasibility.uses_fused()
    rm = mplanner.find_path(q0, q1, interpolation_steps=32)
    assert bool(rm.success.all())
    _check_paths(mplanner, mchecker, rm)


def test_motion_planner_with_graph_planner(device):
    from curobo_amd.motion_planner import MotionPlanner, MotionPlannerCfg
    from curobo_amd.types import JointState

    config = MotionPlannerCfg.create(robot="franka.yml", scene_model={"cuboid": WALL}, num_ik_seeds=32, num_trajopt_seeds=4,
                                     use_graph_planner=True)
    planner = MotionPlanner(config)
    assert planner.graph_planner is not None
    q0, q1 = _wall_problem(device)
    cur = JointState.from_position(q0, planner.joint_names)
    goal = JointState.from_position(q1, planner.joint_names)
    res = planner.plan_cspace(goal, cur, max_attempts=3, enable_graph_attempt=0)
    assert res is not None and bool(res.success.view(-1)[0]), res
    assert planner.graph_planner.n_nodes > 0
    traj = res.js_solution.position.reshape(-1, 7)
    assert bool(planner.graph_planner.checker.validate_trajectory(traj.unsqueeze(0)).all())
    # plan_pose from the first attempt on the roadmap: seed_config (IK) and seed_traj (roadmap paths, possibly fewer than
    # num_trajopt_seeds) go to trajectory optimisation together
    # (a pose whose IK solutions the roadmap joins to the start: the wall problem's four IK goals lie up to 1.8 rad apart and a
    # batched query of all four does not finish within max_path_finding_iterations, so every attempt would be skipped)
    planner.reset_seed()
    assert planner.graph_planner.n_nodes == 0
    near = JointState.from_position(q0.clone(), planner.joint_names)
    near.position[0, 0] += 0.3
    res = planner.plan_pose(planner.compute_kinematics(near).tool_poses.as_goal(), cur, max_attempts=3, enable_graph_attempt=0)
    assert res is not None and bool(res.success.view(-1)[0]), res
    assert planner.graph_planner.n_nodes > 0
    traj = res.js_solution.position.reshape(-1, 7)
    assert bool(planner.graph_planner.checker.validate_trajectory(traj.unsqueeze(0)).all())
    planner.update_world(config.trajopt_solver_config.scene)
    assert planner.graph_planner.n_nodes == 0 and planner.graph_planner.graph.num_edges == 0
    # warmup(enable_graph=True) runs a graph query (its roadmap is emptied afterwards)
    calls = []
    find_path = planner.graph_planner.find_path
    planner.graph_planner.find_path = lambda *a, **k: calls.append(1) or find_path(*a, **k)
    assert planner.warmup(enable_graph=True, num_warmup_iterations=1)
    assert calls and planner.graph_planner.n_nodes == 0
